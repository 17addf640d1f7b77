// emu_galois_seal.cpp -- CPU emulation of the sealed Galois permutation (TEST INFRASTRUCTURE ONLY).
//
// Compiles fhe_reliability_gpu_amd/csrc/galois_seal.hpp -- the per-word step and the per-row verdict the kernels of
// galois_sealed.hip call -- with g++ and runs them over one row cut the way k_automorphism_ntt_sealed cuts it (chunks of
// 2^log_chunk destination words, 256 lanes of two adjacent words per step, the butterfly of the wave shuffles, the four waves, then
// the chunks' partials, last chunk first) followed by k_galois_seal_finish's decision, so that words, seals and flag bits can be
// checked against Python integers without a GPU.  The library never links this file.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I<csrc> emu_galois_seal.cpp -o libemu_galois_seal.so
#include "galois_seal.hpp"

using namespace fhe;

namespace {

template <bool OUT> struct Lanes {
    GalSealAcc<OUT> lane[256];
};

template <bool OUT>
u32 permute_row(const u64 *src, u64 *dst, int logn, u32 k, u64 q, u32 words, const u64 *stored, u64 *seal_dst, u64 *sums, int point, u32 coeff, int bit)
{
    constexpr int W = GalSealAcc<OUT>::WORDS;
    const u32 n = 1u << logn;
    GalSealAcc<OUT> row;
    for (u32 ch = n / words; ch-- > 0;) {
        const u32 j0 = ch * words;
        Lanes<OUT> cur;
        for (u32 t = 0; t < 256; t++)
            for (u32 i = 2 * t; i < words; i += 512)
                for (u32 j = j0 + i; j < j0 + i + 2; j++) {
                    const u64 m = point >= 0 && j == coeff ? (u64)1 << bit : 0;
                    dst[j] = galois_seal_step<OUT>(cur.lane[t], src, j, logn, k, q, point == GAL_AT_WORD ? m : 0, point == GAL_AT_INDEX ? (u32)m : 0u);
                }
        for (u32 o = 32; o; o >>= 1) {      // __shfl_xor inside each wave of 64
            Lanes<OUT> next = cur;
            for (u32 t = 0; t < 256; t++) {
                u64 other[W];
                for (int i = 0; i < W; i++) other[i] = cur.lane[t ^ o].get(i);
                next.lane[t].merge(other);
            }
            cur = next;
        }
        GalSealAcc<OUT> part = cur.lane[0];
        for (u32 w = 1; w < 4; w++) {
            u64 other[W];
            for (int i = 0; i < W; i++) other[i] = cur.lane[64 * w].get(i);
            part.merge(other);
        }
        u64 mem[W];
        for (int i = 0; i < W; i++) mem[i] = part.get(i);
        row.merge(mem);
    }
    sums[0] = seal_canonical(row.s0);
    sums[1] = seal_canonical(row.s1_in);
    sums[2] = OUT ? seal_canonical(row.s1_out) : 0;
    sums[3] = row.over;
    return galois_seal_finish<OUT>(row, stored, seal_dst);
}

} // namespace

extern "C" {

u32 emu_gs_slot(u32 j, int logn, u32 k) { return galois_slot(j, logn, k); }

// dst = sigma_k(src) over one row of 2^logn words (logn >= 1, log_chunk <= logn, 2^log_chunk >= 2) of limb modulus q; stored = the
// source's seal as it lies in memory; out != 0: seal_dst receives the destination's seal (untouched otherwise); sums = the row's
// canonical {s0, s1_in, s1_out, count of words >= q}; fault: point < 0 none, else (point, destination word, bit).  Returns the flags
u32 emu_gs_permute(const u64 *src, u64 *dst, int logn, u32 k, u64 q, int log_chunk, const u64 *stored, int out, u64 *seal_dst, u64 *sums, int point, u32 coeff,
                   int bit)
{
    const u32 words = 1u << log_chunk;
    return out ? permute_row<true>(src, dst, logn, k, q, words, stored, seal_dst, sums, point, coeff, bit)
               : permute_row<false>(src, dst, logn, k, q, words, stored, seal_dst, sums, point, coeff, bit);
}

// the reference sweep of seal_check.hpp over a row in index order: seal = {S0, S1}; returns fhe_seal_verify's flag bits against stored
u32 emu_gs_seal(const u64 *x, u32 n, u64 q, u64 *seal, const u64 *stored)
{
    SealAcc a;
    bool over = false;
    for (u32 j = 0; j < n; j++) {
        a.add(x[j], j);
        over |= x[j] >= q;
    }
    seal[0] = seal_canonical(a.s0);
    seal[1] = seal_canonical(a.s1);
    u32 f = over ? (u32)SEAL_RANGE : 0u;
    if (stored && (seal[0] != stored[0] || seal[1] != stored[1])) f |= (u32)SEAL_SUM;
    return f;
}

// residue_check.hpp: are x and y the same modulo 2^32 - 1, as the checked permutation sees them
int emu_gs_fold32_equal(u64 x, u64 y) { return res_eq(res64(x), res64(y)) ? 1 : 0; }

} // extern "C"
