// ks_seal.hpp -- the inner product of the key switch with the switching key verified on the load that multiplies it (host +
// device: the kernels of keyswitch_sealed.hip and the CPU emulation tests/emu/emu_ks_seal.cpp compile the same functions).
//
// The key [dnum][2][M][N] is the largest and longest-lived operand of every sealed call.  The sealed composites verify it by a
// sweep of its own and k_ks_mac_checked then loads it a second time: a word that is wrong on that second load only passes the
// seal, is a perfectly consistent operand to the residue identity of residue_check.hpp, and pollutes both halves of the result
// with no flag.  The inner product loads every key word exactly once, so the seal of seal_check.hpp (S0 = sum x_j, S1 = sum (j + 1)
// x_j modulo p = 2^61 - 1, and the window x_j < q) is digested from the very register that is then handed to D::mac -- no second
// sweep, and the verified load IS the consuming load.  Per row j a lane keeps one SealAcc per (digit d, half h) (SealRows<2 ND>); a
// row's digests are held against the stored seal of key row (d 2 + h) M + j after the sweep (seal_differs).
//
// The arithmetic is k_ks_mac_checked's, unchanged: KsDotU64 / KsDotF64 over the same terms in the same order d = 0 .. dnum - 1,
// the same finish, the same two fault points per half and the same residue flags; the words are fhe_keyswitch_apply's bit for bit
// -- also for a key word that is not canonical: the call flags such a word (the window bit here, PW_OPERAND in the residue flags),
// it does not fix it.  The d loop is unrolled to the compile-time bound ND (guarded by d < dnum), so that the accumulators are
// indexed by constants and stay in registers, and the term numbers of the folds are constants as well.
//
// What a raised key word means: SEAL_SUM -- the row as it was loaded for this product is not the row that was sealed (one or two
// changed words: with certainty, seal_check.hpp), or a stored sum is not canonical; SEAL_RANGE -- a loaded word is >= q_j.  Integer
// arithmetic modulo p throughout: no digest depends on how a row is cut into chunks, lanes or waves, nor on the order in which
// partial sums are merged.
#pragma once
#include "residue_check.hpp"
#include "seal_check.hpp"

namespace fhe {

// the largest dnum the fused kernel is instantiated for; beyond it a verifying sweep precedes the checked inner product
constexpr u32 KS_SEAL_MAX_DNUM = 12;

// the one-shot test fault of fhe_ctx_inject_fault_keyswitch_sealed as one row's job reads it: XOR mask into word coeff of half h of
// digit d of this row's key words, in the register as loaded -- before both the digest and the product read it (mask == 0: not
// this row)
struct KsHit {
    u32 d, h;
    u64 coeff, mask;
};

// Two adjacent words j, j + 1 of row p: ld(d, x, k0, k1) loads the two words of digit d (the owned limb or its extension, as
// k_ks_mac_checked chooses) and of both key halves.  Digests every key word into g (row 2 d + h = half h of digit d < ND), forms
// the two words of each half of the sums and ORs their residue flags into fl0 / fl1.  f0 / f1 = the checked call's test fault for
// word j and word j + 1 of half 0 / half 1.
template <class D, int ND, bool HOOK, class LD>
FHE_HD void ks_seal_pair(SealRows<2 * ND> &g, u32 dnum, u32 j, const LimbParams &p, const LD &ld, const KsHit &hit, const PwFault *f0, const PwFault *f1, u64 *c0,
                         u64 *c1, u32 &fl0, u32 &fl1)
{
    D s0x, s1x, s0y, s1y;      // half 0 / 1 of word j (x) and of word j + 1 (y)
    seal_each<0, ND>([&](auto dc) {
        constexpr int d = decltype(dc)::value;
        if ((u32)d < dnum) {
            u64 x[2], k0[2], k1[2];
            ld((u32)d, x, k0, k1);
            if (HOOK && (u32)d == hit.d) {
                u64 *k = hit.h ? k1 : k0;
                k[0] ^= j == hit.coeff ? hit.mask : 0;
                k[1] ^= (u64)j + 1 == hit.coeff ? hit.mask : 0;
            }
            g.acc[2 * d].add(k0[0], j);
            g.acc[2 * d].add(k0[1], j + 1);
            g.acc[2 * d + 1].add(k1[0], j);
            g.acc[2 * d + 1].add(k1[1], j + 1);
            g.range |= ((k0[0] >= p.q || k0[1] >= p.q) ? 1u << (2 * d) : 0u) | ((k1[0] >= p.q || k1[1] >= p.q) ? 2u << (2 * d) : 0u);
            s0x.mac(x[0], k0[0], (u32)d, p, f0[0]);
            s1x.mac(x[0], k1[0], (u32)d, p, f1[0]);
            s0y.mac(x[1], k0[1], (u32)d, p, f0[1]);
            s1y.mac(x[1], k1[1], (u32)d, p, f1[1]);
        }
    });
    u32 a, b, c, e;
    c0[0] = s0x.finish(dnum, p, a, f0[0]);
    c1[0] = s1x.finish(dnum, p, b, f1[0]);
    c0[1] = s0y.finish(dnum, p, c, f0[1]);
    c1[1] = s1y.finish(dnum, p, e, f1[1]);
    fl0 |= a | c;
    fl1 |= b | e;
}

// the names tests/emu/emu_ks_seal.cpp knows the record ([d][h]: row 2 d + h) and the finish step's decision by
template <int ND> using KsSeal = SealRows<2 * ND>;
FHE_HD bool ks_seal_decide(u64 s0, u64 s1, const u64 *stored) { return seal_differs(s0, s1, stored); }

} // namespace fhe
