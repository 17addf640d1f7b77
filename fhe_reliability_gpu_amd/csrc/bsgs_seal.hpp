// bsgs_seal.hpp -- the inner sum of the BSGS product with its diagonals verified on the load that uses them (host + device: the
// kernels of bsgs_sealed.hip and the CPU emulation tests/emu/emu_bsgs_seal.cpp compile the same functions).
//
// The diagonals [n2][n1][L][N] are the largest and longest-lived operand of the product, and a word that rots in one is a perfectly
// consistent operand to the residue identity of bsgs_check.hpp: no flag, wrong product.  The inner sum loads every diagonal word
// exactly once, so its seal (seal_check.hpp: S0 = sum x_j, S1 = sum (j + 1) x_j modulo p = 2^61 - 1, and the window x_j < q) is
// digested from the very register that is then handed to DiagDot::mac -- no second sweep, and the verified load IS the consuming
// load.  Per giant step g and limb row l a lane keeps one SealAcc per baby step b < n1 (SealRows<NB>); a row's digests are held
// against the stored seal seal_diag[(g n1 + b) L + l] after the sweep (seal_differs).
//
// The arithmetic is k_diag_mac_checked's, unchanged: DiagDot<KsDotU64 / KsDotF64> over the same terms in the same order, folds
// after every eighth term, the same four fault points and residue flags; the words are fhe_bsgs_matvec's bit for bit.  The b loop
// is unrolled to the compile-time bound NB (guarded by b < n1), so that the accumulators are indexed by constants and stay in
// registers, and the term numbers of the folds are constants as well.
//
// What a raised word means: SEAL_SUM -- the row as it was loaded for this product is not the row that was sealed (one or two
// changed words: with certainty, seal_check.hpp), or a stored sum is not canonical; SEAL_RANGE -- a loaded word is >= q_l (the
// residue check then raises PW_OPERAND on both parts as before).  Integer arithmetic modulo p throughout: no digest depends on how
// a row is cut into chunks, lanes or waves.
#pragma once
#include "bsgs_check.hpp"
#include "seal_check.hpp"

namespace fhe {

// the largest n1 the fused kernel is instantiated for; beyond it a verifying sweep precedes the checked inner sum
constexpr u32 DIAG_SEAL_MAX_NB = 16;

// the one-shot test fault of fhe_ctx_inject_fault_bsgs_sealed as a launch reads it: XOR mask into word coeff of row `limb` of
// diagonal b, in the register as loaded -- before both the digest and the product read it (mask == 0: not armed)
struct DiagHit {
    u32 b, limb;
    u64 coeff, mask;
};

// Two adjacent words j, j + 1 of limb row p: ld(b, d, y0, y1) loads the diagonal words of baby step b and the words of both parts
// of the b-th rotated ciphertext.  Digests every diagonal word into g (row b = diagonal b < NB), forms the two words of each part
// (c0, c1) and ORs their residue flags into fl0 / fl1.  f0 / f1 = the checked call's test fault for word j and word j + 1 of part
// 0 / part 1.
template <class D, int NB, bool HOOK, class LD>
FHE_HD void diag_seal_pair(SealRows<NB> &g, u32 n1, u32 j, const LimbParams &p, const LD &ld, const DiagHit &hit, const PwFault *f0, const PwFault *f1, u64 *c0,
                           u64 *c1, u32 &fl0, u32 &fl1)
{
    DiagDot<D> sx, sy;
    seal_each<0, NB>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        if ((u32)b < n1) {
            u64 d[2], y0[2], y1[2];
            ld((u32)b, d, y0, y1);
            if (HOOK && (u32)b == hit.b) {
                d[0] ^= j == hit.coeff ? hit.mask : 0;
                d[1] ^= (u64)j + 1 == hit.coeff ? hit.mask : 0;
            }
            g.acc[b].add(d[0], j);
            g.acc[b].add(d[1], j + 1);
            g.range |= (d[0] >= p.q || d[1] >= p.q) ? 1u << b : 0u;
            sx.mac(d[0], y0[0], y1[0], (u32)b, p, f0[0], f1[0]);
            sy.mac(d[1], y0[1], y1[1], (u32)b, p, f0[1], f1[1]);
        }
    });
    u32 x0, x1, z0, z1;
    sx.finish(n1, p, c0[0], c1[0], x0, x1, f0[0], f1[0]);
    sy.finish(n1, p, c0[1], c1[1], z0, z1, f0[1], f1[1]);
    fl0 |= x0 | z0;
    fl1 |= x1 | z1;
}

// the names tests/emu/emu_bsgs_seal.cpp knows the record and the finish step's decision by
template <int NB> using DiagSeal = SealRows<NB>;
FHE_HD bool diag_seal_decide(u64 s0, u64 s1, const u64 *stored) { return seal_differs(s0, s1, stored); }

} // namespace fhe
