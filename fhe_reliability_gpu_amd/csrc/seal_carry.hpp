// seal_carry.hpp -- seals carried through a modular add or subtract (host + device: the kernels of seal_carry.hip and the CPU
// emulation tests/emu/emu_seal_carry.cpp compile the same functions).
//
// The seal of seal_check.hpp is linear, and so is the operation.  With canonical operands the add is c_j = a_j + b_j - e_j q with
// the wrap bit e_j in {0, 1}, an identity between integers, so for i = 0, 1, 2 and the weights w_j = j + 1
//     S_i(c) = S_i(a) + S_i(b) - q E_i   (mod p = 2^61 - 1),      E_i = sum_j w_j^i e_j,
// and the subtract c_j = a_j - b_j + e_j q gives S_i(c) = S_i(a) - S_i(b) + q E_i.  One sweep loads each operand word once, forms
// c, counts the wraps, and digests c from the register it is about to store; a row's digest is then held against the value
// PREDICTED from the seals the operands came with.  What differs between the two:
//   a word of a or b that is not the word that was sealed: c moves by d with 0 < |d| < q < p whatever the wrap does (the wrap is
//     counted as it happened), the prediction does not;
//   a fault in the adder: the digest moves, the prediction does not;
//   a fault in the wrap count: the prediction moves by q w^i, not zero modulo p because q < p and w <= N < p.
// The seal written for c is the predicted one, matched or not.  A fault after the digest (the store, memory) is therefore seen by
// whoever verifies c next, and a row that was raised once stays raised through every later carried operation: its words and its
// seal differ by the same amount ever after.
//
// An operand word >= q is reduced exactly as k_modadd / k_modsub reduce it (barrett128; the word itself when canonical), which
// leaves the identity above: the row raises SEAL_RANGE, and SEAL_SUM as well where the word that was sealed was canonical -- the
// reduced word differs from it by less than q.
//
// Wrap sums: E0 <= N and E1 <= N (N + 1) / 2 need no reduction below N = 2^30; the square (j + 1)^2 passes 2^32 from N = 2^17 on but
// stays below 2^64 as a 64-bit product of 32-bit weights, and is folded before it is added.  All sums are kept lazily reduced (at
// most p + 7) as in seal_check.hpp and made canonical once, per row.
#pragma once
#include <type_traits>

#include "residue_check.hpp"
#include "seal_check.hpp"

namespace fhe {

// injection points of the one-shot test hook (fhe_ctx_inject_fault_seal_carry): a word of a / of b after its load, c before the
// digest and the store, c after the digest and before the store, the wrap bit as counted
enum { CARRY_AT_A = 0, CARRY_AT_B = 1, CARRY_AT_C = 2, CARRY_AT_STORE = 3, CARRY_AT_WRAP = 4 };

// what one row (or one lane, one chunk) has accumulated: the digest of c and the weighted wrap counts; s2 / e2 only with a locator
template <bool LOC> struct CarryAcc {
    static constexpr int WORDS = LOC ? 6 : 4;      // {s0, s1, [s2], e0, e1, [e2]}: a job's partials
    typename std::conditional<LOC, SealAcc3, SealAcc>::type c;
    u64 e0 = 0, e1 = 0, e2 = 0;

    // one element at index j of its row: returns the word to store; range |= an operand was not canonical
    template <bool SUB> FHE_HD u64 step(u64 a, u64 b, u64 q, u64 r0, u64 r1, u32 j, const PwFault &f, bool &range)
    {
        a = pw_hit(a, f, CARRY_AT_A);
        b = pw_hit(b, f, CARRY_AT_B);
        if (a >= q || b >= q) {
            range = true;
            a = barrett128(a, 0, q, r0, r1);
            b = barrett128(b, 0, q, r0, r1);
        }
        u64 w;
        bool e;
        if (SUB) {
            e = a < b;
            w = e ? a + q - b : a - b;
        } else {
            const u64 s = a + b;
            e = s >= q;
            w = e ? s - q : s;
        }
        w = pw_hit(w, f, CARRY_AT_C);
        if (f.point == CARRY_AT_WRAP && f.mask) e = !e;
        const u32 wt = j + 1;
        c.add(w, j);
        if (LOC) e2 = seal_fold(e2 + (e ? seal_fold((u64)wt * wt) : 0));
        e0 += e ? 1 : 0;
        e1 += e ? wt : 0;
        return pw_hit(w, f, CARRY_AT_STORE);
    }

    // the sums as they travel (shuffles, LDS, the partials in memory): WORDS of them, in the order of a job's partials
    FHE_HD u64 get(int i) const
    {
        if constexpr (LOC) return i == 0 ? c.s0 : i == 1 ? c.s1 : i == 2 ? c.s2 : i == 3 ? e0 : i == 4 ? e1 : e2;
        else return i == 0 ? c.s0 : i == 1 ? c.s1 : i == 2 ? e0 : e1;
    }
    FHE_HD void merge(const u64 *o)
    {
        if constexpr (LOC) c.merge(o[0], o[1], o[2]);
        else c.merge(o[0], o[1]);
        e0 = seal_fold(e0 + seal_fold(o[LOC ? 3 : 2]));
        e1 = seal_fold(e1 + seal_fold(o[LOC ? 4 : 3]));
        if (LOC) e2 = seal_fold(e2 + seal_fold(o[5]));
    }
};

// the canonical sum S_i(c) predicted from the stored sums sa, sb of the operands (any 64-bit words) and the wrap sum E (lazily
// reduced): sa + sb - q E for the add, sa - sb + q E for the subtract.  q < p always holds here (q = 1 modulo 2 N, p is not), so
// seal_mulmod's operands are canonical
FHE_HD u64 carry_predict(u64 sa, u64 sb, u64 q, u64 E, bool sub)
{
    const u64 a = seal_canonical(sa), b = seal_canonical(sb), t = seal_mulmod(q, seal_canonical(E));
    return seal_canonical(sub ? a + (SEAL_P - b) + t : a + b + (SEAL_P - t));
}

// what the finish step decides for one row: got = the lazily reduced digest of c, E = the wrap sums, sa / sb = the operands' stored
// sums {S0, S1, [S2]}; pred receives the canonical sums to store.  True where the row is to raise SEAL_SUM: a digest differs from
// its prediction, or a stored sum is not canonical (fhe_seal_verify holds stored sums word for word, and so does this)
template <bool LOC> FHE_HD bool carry_finish(const u64 *got, const u64 *E, const u64 *sa, const u64 *sb, u64 q, bool sub, u64 *pred)
{
    bool bad = false;
    for (int i = 0; i < (LOC ? 3 : 2); i++) {
        pred[i] = carry_predict(sa[i], sb[i], q, E[i], sub);
        bad |= seal_canonical(got[i]) != pred[i] || sa[i] >= SEAL_P || sb[i] >= SEAL_P;
    }
    return bad;
}

} // namespace fhe
