// emu_bsgs_seal.cpp -- CPU emulation of the sealed inner sum of the BSGS product (TEST INFRASTRUCTURE ONLY).
//
// Compiles fhe_reliability_gpu_amd/csrc/bsgs_seal.hpp -- the per-pair step and the per-row decision the kernels of bsgs_sealed.hip
// call -- with g++ and runs one limb row's job loop the way k_diag_mac_sealed runs it (chunks of 2^log_chunk words, 256 lanes of two
// adjacent words per step, NB accumulators per lane, the butterfly of the wave shuffles, the four waves, then the chunks' partials)
// followed by k_diag_seal_finish's decision per baby step, so that words, digests and flag bits can be checked against Python
// integers without a GPU.  The library never links this file.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I<csrc> emu_bsgs_seal.cpp -o libemu_bsgs_seal.so
#include "bsgs_seal.hpp"

using namespace fhe;

namespace {

// the limb constants as capi.cpp build_tables fills them (the fields these elements read)
LimbParams limb(u64 q, int path)
{
    LimbParams p{};
    p.q = q;
    p.two_q = 2 * q;
    p.n = (double)q;
    p.ninv = 1.0 / p.n;
    const unsigned __int128 ratio = ~(unsigned __int128)0 / q;      // floor(2^128 / q) for q not a power of two
    p.barrett_lo = (u64)ratio;
    p.barrett_hi = (u64)(ratio >> 64);
    p.path = path;
    return p;
}

template <int NB> struct Lanes {
    DiagSeal<NB> lane[256];
};

template <class D, int NB>
void sealed_row(const u64 *d, const u64 *y0, const u64 *y1, u32 n1, u32 n, const LimbParams &p, u32 words, const u64 *seal, const DiagHit &hit, u64 *w0, u64 *w1,
                u32 *fl, u64 *digest, u32 *seal_flags)
{
    const PwFault none[2] = {PwFault{-1, 0}, PwFault{-1, 0}};
    SealAcc row[NB];
    u32 range = 0;
    fl[0] = fl[1] = 0;
    for (u32 ch = n / words; ch-- > 0;) {
        const u32 j0 = ch * words;
        Lanes<NB> cur;
        for (u32 t = 0; t < 256; t++)
            for (u32 i = 2 * t; i < words; i += 512) {
                const u32 j = j0 + i;
                auto ld = [&](u32 b, u64 *dd, u64 *a0, u64 *a1) {
                    for (int w = 0; w < 2; w++) {
                        dd[w] = d[(size_t)b * n + j + w];
                        a0[w] = y0[(size_t)b * n + j + w];
                        a1[w] = y1[(size_t)b * n + j + w];
                    }
                };
                if (hit.mask) diag_seal_pair<D, NB, true>(cur.lane[t], n1, j, p, ld, hit, none, none, w0 + j, w1 + j, fl[0], fl[1]);
                else diag_seal_pair<D, NB, false>(cur.lane[t], n1, j, p, ld, hit, none, none, w0 + j, w1 + j, fl[0], fl[1]);
            }
        for (u32 o = 32; o; o >>= 1) {      // __shfl_xor inside each wave of 64
            Lanes<NB> next = cur;
            for (u32 t = 0; t < 256; t++) {
                for (int b = 0; b < NB; b++) next.lane[t].acc[b].merge(cur.lane[t ^ o].acc[b].s0, cur.lane[t ^ o].acc[b].s1);
                next.lane[t].range |= cur.lane[t ^ o].range;
            }
            cur = next;
        }
        for (u32 w = 1; w < 4; w++) {
            for (int b = 0; b < NB; b++) cur.lane[0].acc[b].merge(cur.lane[64 * w].acc[b].s0, cur.lane[64 * w].acc[b].s1);
            cur.lane[0].range |= cur.lane[64 * w].range;
        }
        // the chunk's partial, then k_diag_seal_finish's sum over the chunks
        for (int b = 0; b < NB; b++) row[b].merge(cur.lane[0].acc[b].s0, cur.lane[0].acc[b].s1);
        range |= cur.lane[0].range;
    }
    for (u32 b = 0; b < n1; b++) {
        digest[2 * b] = seal_canonical(row[b].s0);
        digest[2 * b + 1] = seal_canonical(row[b].s1);
        seal_flags[b] = (range >> b & 1 ? (u32)SEAL_RANGE : 0u) | (diag_seal_decide(row[b].s0, row[b].s1, seal + 2 * b) ? (u32)SEAL_SUM : 0u);
    }
}

template <class D>
int sealed_nb(const u64 *d, const u64 *y0, const u64 *y1, u32 n1, u32 n, const LimbParams &p, u32 words, const u64 *seal, const DiagHit &hit, u64 *w0, u64 *w1,
              u32 *fl, u64 *digest, u32 *seal_flags)
{
    if (n1 <= 4) sealed_row<D, 4>(d, y0, y1, n1, n, p, words, seal, hit, w0, w1, fl, digest, seal_flags);
    else if (n1 <= 8) sealed_row<D, 8>(d, y0, y1, n1, n, p, words, seal, hit, w0, w1, fl, digest, seal_flags);
    else sealed_row<D, 16>(d, y0, y1, n1, n, p, words, seal, hit, w0, w1, fl, digest, seal_flags);
    return 0;
}

} // namespace

extern "C" {

// One limb row of n words (n a multiple of 2^log_chunk >= 2) of a giant step with n1 <= 16 baby steps: d = [n1][n] diagonal words,
// y0 / y1 = [n1][n] words of the two parts, seal = [n1][2] the stored seals of the diagonal rows; path 0 = FP64-term form, 1 = U64.
// hit_bit >= 0: bit hit_bit of diagonal word (hit_b, hit_coeff) is flipped in the register as loaded.  Out: the words of both
// parts, fl[2] = the OR of each part's residue flags, digest = [n1][2] canonical sums of the rows as loaded, seal_flags = [n1]
int emu_diag_mac_sealed(const u64 *d, const u64 *y0, const u64 *y1, int n1, u32 n, u64 q, int path, int log_chunk, const u64 *seal, int hit_b, u32 hit_coeff,
                        int hit_bit, u64 *w0, u64 *w1, u32 *fl, u64 *digest, u32 *seal_flags)
{
    if (n1 < 1 || n1 > (int)DIAG_SEAL_MAX_NB || (path == PATH_F64 && q >= ((u64)1 << 50)) || log_chunk < 1 || n % (1u << log_chunk)) return -1;
    const LimbParams p = limb(q, path);
    const DiagHit hit{(u32)hit_b, 0u, hit_coeff, hit_bit >= 0 ? (u64)1 << hit_bit : 0};
    const u32 words = 1u << log_chunk;
    if (path == PATH_F64) return sealed_nb<KsDotF64>(d, y0, y1, (u32)n1, n, p, words, seal, hit, w0, w1, fl, digest, seal_flags);
    return sealed_nb<KsDotU64>(d, y0, y1, (u32)n1, n, p, words, seal, hit, w0, w1, fl, digest, seal_flags);
}

} // extern "C"
