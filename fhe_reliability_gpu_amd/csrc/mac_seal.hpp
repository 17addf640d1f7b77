// mac_seal.hpp -- the two-half inner product with its long-lived operand verified on the load that multiplies it (host + device:
// the kernels of mac_sealed.hip and, under the families' own names in ks_seal.hpp and bsgs_seal.hpp, the CPU emulations
// tests/emu/emu_ks_seal.cpp and tests/emu/emu_bsgs_seal.cpp compile the same functions).  Two families run it: the key switch's
// inner product over the digits, sealed operand the switching key [dnum][2][M][N], and the BSGS product's inner sum over the baby
// steps, sealed operand the diagonals [n2][n1][L][N].
//
// Either operand is the largest and longest-lived of its call, and a word that rots in it is a perfectly consistent operand to the
// residue identity of residue_check.hpp: no flag, wrong product -- also when a sweep of its own has verified it before, because the
// product then loads it a second time.  The inner product loads every such word exactly once, so its seal (seal_check.hpp: S0 = sum
// x_j, S1 = sum (j + 1) x_j modulo p = 2^61 - 1, and the window x_j < q) is digested from the very register that is then handed to
// D::mac -- no second sweep, and the verified load IS the consuming load.  Per row and term a lane keeps one SealAcc per sealed row
// the term reads (SealRows<ROWS T>); a row's digests are held against its stored seal after the sweep (seal_differs).
//
// The arithmetic is the checked kernels', unchanged (k_ks_mac_checked, k_diag_mac_checked): per word and half one KsDotU64 /
// KsDotF64 over the same terms in the same order, folds after every eighth term, the same finish, the same fault points and residue
// flags; the words are the unchecked calls' bit for bit -- also for a sealed word that is not canonical: the call flags such a word
// (the window bit here, PW_OPERAND in the residue flags), it does not fix it.  The term loop is unrolled to the compile-time bound T
// (guarded by the run-time count), so that the accumulators are indexed by constants and stay in registers, and the term numbers of
// the folds are constants as well.
//
// What a raised word means: SEAL_SUM -- the row as it was loaded for this product is not the row that was sealed (one or two
// changed words: with certainty, seal_check.hpp), or a stored sum is not canonical; SEAL_RANGE -- a loaded word is >= q.  Integer
// arithmetic modulo p throughout: no digest depends on how a row is cut into chunks, lanes or waves, nor on the order in which
// partial sums are merged.
#pragma once
#include "residue_check.hpp"
#include "seal_check.hpp"

namespace fhe {

// the largest dnum / n1 the fused kernel is instantiated for; beyond it a verifying sweep precedes the checked inner product
constexpr u32 KS_SEAL_MAX_DNUM = 12;
constexpr u32 DIAG_SEAL_MAX_NB = 16;

// A term loads three pairs of words: u, the first operand of both halves' products, and v0 / v1, the second operand of half 0 / 1
// (the order matters: the FP64 quotient estimate a (b / q) is not symmetric).  What a family states is which of them are sealed:
// ROWS = 2, the key switch -- u is the digit, v0 / v1 are the two key halves, sealed rows 2 d + h of term d;
// ROWS = 1, the BSGS inner sum -- u is the diagonal, sealed row b of term b, v0 / v1 are the two parts of the b-th rotated ciphertext
struct KsSealFamily {
    static constexpr int ROWS = 2;
};
struct DiagSealFamily {
    static constexpr int ROWS = 1;
};

// the sealed call's one-shot test fault as one job reads it: XOR mask into word coeff of sealed row `slot` of this job's rows, in
// the register as loaded -- before both the digest and the product read it (mask == 0: not this job)
struct MacSealHit {
    u32 slot;
    u64 coeff, mask;
};

// Two adjacent words j, j + 1 of a row with limb constants p: ld(t, u, v0, v1) loads the two words of each operand of term t < T.
// Digests every sealed word into g, forms the two words of each half of the sums (c0, c1) and ORs their residue flags into fl0 /
// fl1.  f0 / f1 = the checked call's test fault for word j and word j + 1 of half 0 / half 1.
template <class D, class Family, int T, bool HOOK, class LD>
FHE_HD void mac_seal_pair(SealRows<Family::ROWS * T> &g, u32 terms, u32 j, const LimbParams &p, const LD &ld, const MacSealHit &hit, const PwFault *f0,
                          const PwFault *f1, u64 *c0, u64 *c1, u32 &fl0, u32 &fl1)
{
    constexpr int R = Family::ROWS;
    D s0x, s1x, s0y, s1y;      // half 0 / 1 of word j (x) and of word j + 1 (y)
    seal_each<0, T>([&](auto tc) {
        constexpr int t = decltype(tc)::value;
        if ((u32)t < terms) {
            u64 u[2], v0[2], v1[2];
            ld((u32)t, u, v0, v1);
            if (HOOK && hit.slot / R == (u32)t) {
                u64 *w = R == 1 ? u : hit.slot % R ? v1 : v0;
                w[0] ^= j == hit.coeff ? hit.mask : 0;
                w[1] ^= (u64)j + 1 == hit.coeff ? hit.mask : 0;
            }
            seal_each<0, R>([&](auto rc) {
                constexpr int r = decltype(rc)::value, slot = R * t + r;
                const u64 *w = R == 1 ? u : r ? v1 : v0;
                g.acc[slot].add(w[0], j);
                g.acc[slot].add(w[1], j + 1);
                g.range |= (w[0] >= p.q || w[1] >= p.q) ? 1u << slot : 0u;
            });
            s0x.mac(u[0], v0[0], (u32)t, p, f0[0]);
            s1x.mac(u[0], v1[0], (u32)t, p, f1[0]);
            s0y.mac(u[1], v0[1], (u32)t, p, f0[1]);
            s1y.mac(u[1], v1[1], (u32)t, p, f1[1]);
        }
    });
    u32 a, b, c, e;
    c0[0] = s0x.finish(terms, p, a, f0[0]);
    c1[0] = s1x.finish(terms, p, b, f1[0]);
    c0[1] = s0y.finish(terms, p, c, f0[1]);
    c1[1] = s1y.finish(terms, p, e, f1[1]);
    fl0 |= a | c;
    fl1 |= b | e;
}

} // namespace fhe
