// emu_galois_check.cpp -- CPU emulation of the checked NTT-domain Galois permutation (TEST INFRASTRUCTURE ONLY).
//
// Compiles fhe_reliability_gpu_amd/csrc/galois_check.hpp -- the element functions the kernel of galois_checked.hip calls --
// with g++ and runs them over rows of words, with an optional bit flip at one injection point of one element, so that words,
// sums and flags can be checked against Python integers without a GPU.  The library never links this file.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I<csrc> emu_galois_check.cpp -o libemu_galois_check.so
#include "galois_check.hpp"

using namespace fhe;

extern "C" {

u32 emu_galois_slot(u32 j, int logn, u32 k) { return galois_slot(j, logn, k); }

// dst[u][j] = src[u][pi_k(j)] for n_units rows of 2^logn words, the units' two sums and flags as the kernel forms them: every
// position j of a row runs the destination side (gather, store, term of s_out) and the source side (linear read, term of s_in).
// point >= 0: the test fault at (unit, coeff), bit `bit`
int emu_galois_permute(const u64 *src, size_t n_units, int logn, u32 k, u32 kinv, int point, u32 unit, u64 coeff, int bit, u64 *dst,
                       u64 *s_in, u64 *s_out, u32 *flags)
{
    if (logn < 1 || logn > 30 || !(k & 1) || !(kinv & 1)) return -1;
    if (point >= 0 && (!galois_point_exists(point, bit, logn) || unit >= n_units || coeff >> logn)) return -1;
    const u64 n = (u64)1 << logn;
    for (size_t u = 0; u < n_units; u++) {
        u64 in = 0, out = 0;
        for (u64 j = 0; j < n; j++) {
            const bool hit = point >= 0 && u == unit && j == coeff;
            u64 t_out;
            dst[u * n + j] = galois_gather(src + u * n, (u32)j, logn, k, hit && point == GAL_AT_WORD ? (u64)1 << bit : 0,
                                           hit && point == GAL_AT_INDEX ? 1u << bit : 0u, t_out);
            out += t_out;
            in += galois_source_term(src[u * n + j], (u32)j, logn, kinv);
        }
        s_in[u] = in;
        s_out[u] = out;
        flags[u] = galois_sums_flag(in, out);
    }
    return 0;
}

} // extern "C"
