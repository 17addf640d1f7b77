// emu_seal_carry.cpp -- CPU emulation of the carried add / subtract (TEST INFRASTRUCTURE ONLY).
//
// Compiles fhe_reliability_gpu_amd/csrc/seal_carry.hpp -- the per-word step and the per-row prediction the kernels of seal_carry.hip
// call -- with g++ and runs them over one row cut the way k_modadd_carry cuts it (chunks of 2^log_chunk words, 256 lanes of two
// adjacent words per load, the butterfly of the wave shuffles, the four waves, then the chunks' partials, last chunk first) followed
// by k_modadd_carry_finish's decision, so that words, predicted sums and flag bits can be checked against Python integers without a
// GPU.  The library never links this file.
//
//   g++ -O2 -std=c++17 -shared -fPIC -I<csrc> emu_seal_carry.cpp -o libemu_seal_carry.so
#include "seal_carry.hpp"

using namespace fhe;

namespace {

template <bool LOC> struct Lanes {
    CarryAcc<LOC> lane[256];
};

// one row; returns the flag bits.  fault: point < 0 none, else (point, coeff, bit)
template <bool SUB, bool LOC>
u32 carry_row(const u64 *a, const u64 *b, u64 *c, u32 n, u64 q, u32 words, const u64 *sa, const u64 *sb, u64 *pred, int point, u32 coeff, int bit)
{
    constexpr int W = CarryAcc<LOC>::WORDS, S = LOC ? 3 : 2;
    const unsigned __int128 ratio = ~(unsigned __int128)0 / q;      // floor(2^128 / q): q is odd
    const u64 r0 = (u64)ratio, r1 = (u64)(ratio >> 64);
    bool range = false;
    CarryAcc<LOC> row;
    for (u32 ch = n / words; ch-- > 0;) {
        const u32 j0 = ch * words;
        Lanes<LOC> cur;
        for (u32 t = 0; t < 256; t++)
            for (u32 i = 2 * t; i < words; i += 512)
                for (u32 j = j0 + i; j < j0 + i + 2; j++) {
                    const PwFault f{point >= 0 ? point : -1, point >= 0 && j == coeff ? (u64)1 << bit : 0};
                    c[j] = cur.lane[t].template step<SUB>(a[j], b[j], q, r0, r1, j, f, range);
                }
        for (u32 o = 32; o; o >>= 1) {      // __shfl_xor inside each wave of 64
            Lanes<LOC> next = cur;
            for (u32 t = 0; t < 256; t++) {
                u64 other[W];
                for (int i = 0; i < W; i++) other[i] = cur.lane[t ^ o].get(i);
                next.lane[t].merge(other);
            }
            cur = next;
        }
        CarryAcc<LOC> part = cur.lane[0];
        for (u32 w = 1; w < 4; w++) {
            u64 other[W];
            for (int i = 0; i < W; i++) other[i] = cur.lane[64 * w].get(i);
            part.merge(other);
        }
        u64 stored[W];
        for (int i = 0; i < W; i++) stored[i] = part.get(i);
        row.merge(stored);
    }
    u64 got[S], E[S];
    for (int i = 0; i < S; i++) got[i] = row.get(i), E[i] = row.get(S + i);
    u32 flags = range ? (u32)SEAL_RANGE : 0u;
    if (carry_finish<LOC>(got, E, sa, sb, q, SUB, pred)) flags |= (u32)SEAL_SUM;
    return flags;
}

} // namespace

extern "C" {

// c = a + b (sub = 0) or a - b mod q over one row of n words (n a multiple of 2^log_chunk >= 2); sa, sb = the operands' stored
// {S0, S1, S2}, pred = the sums the finish step stores ([3]; S2 only with loc); returns the row's flag bits
u32 emu_carry(const u64 *a, const u64 *b, u64 *c, u32 n, u64 q, int sub, int loc, int log_chunk, const u64 *sa, const u64 *sb, u64 *pred, int point,
              u32 coeff, int bit)
{
    const u32 words = 1u << log_chunk;
    if (sub) return loc ? carry_row<true, true>(a, b, c, n, q, words, sa, sb, pred, point, coeff, bit)
                        : carry_row<true, false>(a, b, c, n, q, words, sa, sb, pred, point, coeff, bit);
    return loc ? carry_row<false, true>(a, b, c, n, q, words, sa, sb, pred, point, coeff, bit)
               : carry_row<false, false>(a, b, c, n, q, words, sa, sb, pred, point, coeff, bit);
}

u64 emu_carry_predict(u64 sa, u64 sb, u64 q, u64 E, int sub) { return carry_predict(sa, sb, q, E, sub != 0); }

// residue_check.hpp: are x and y the same modulo 2^32 - 1, as the checked products see them
int emu_carry_fold32_equal(u64 x, u64 y) { return res_eq(res64(x), res64(y)) ? 1 : 0; }

} // extern "C"
