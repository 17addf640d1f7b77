// baseconv_check.hpp -- residue-checked RNS base conversion (host + device: the kernels of baseconv_checked.hip and the CPU
// emulation in tests/emu/emu_baseconv.cpp compile the same functions).
//
// Both conversions are sums of products with constants (aux_kernels.hip bc_exact_body / k_bconv_fast; the stage the reference
// perturbs in motivation/baseConv.py and rfhe_framewk/src/baseConv.{py,cpp,cu}):
//     digit j    r_j A_j - sum_{l<j} c_l D_lj = K_j p_j + c_j      0 <= c_j < p_j, K_j signed
//     output o   sum_l c_l E_lo               = K_o q_o + out_o    0 <= out_o < q_o
//     fast o     sum_j in_j C_jo              = K_o q_o + out_o    0 <= out_o < m q_o   (the sum of the reduced terms, not reduced)
// The element functions below form every term as a Shoup product a w = k q + t (0 <= t < q for ANY 64-bit a: k = mulhi(a, w')
// plus the one conditional subtraction), combine the terms with one conditional +- q each, and carry next to the value the
// residue of the total quotient K = sum +-k_l +- (corrections taken) modulo m = 2^32 - 1.  K itself can pass 64 bits (64 terms
// of 64-bit quotients), its residue cannot.  The identity is then checked modulo m with 32-bit lane arithmetic that shares
// nothing with the 64-bit multiplies which made the word (residue_check.hpp: res_*), together with the window of the word.
// Canonical digits and outputs are unique, so the words are those of the unchecked kernels on either arithmetic path of a plan
// (FP64 constants below 2^50, Shoup pairs above): the checked kernels run the Shoup form on both, from Shoup-pair tables.
//
// An intermediate that is out of its window but consistent (a Shoup remainder one q too high that the next conditional step
// absorbs, a digit n p too high with K n too low, n < 64) gives the right word and raises nothing; only the final word has a window.  A digit that is wrong (or >= p_j) is
// used as it is by the later digits and by every output: their identities hold for the digit they were given, so a fault is
// flagged on the unit it hit and on no other.  Not covered: faults already in the input words, a register fault on a digit
// between its check and a later use, faults in the plan's constant tables.
//
// Injection points (residue_check.hpp PW_AT_*): PRODUCT = low word of the first term's 128-bit product; QUOTIENT = the Shoup
// quotient of the reduction that completes the digit / word (its last term; the fast form, which has no closing reduction:
// the first term's); RESULT = the digit / word before its window check and every later use; SUM = the running sum with its
// last term folded in, before the conditional +- q that closes it (fast form: the sum of all terms but the last).  SUM needs
// two terms: it does not exist on digit 0, nor on outputs when m = 1.
#pragma once
#include "residue_check.hpp"

namespace fhe {

// a w mod q with the residue of its quotient: a w = k q + t over the integers, 0 <= t < q for any 64-bit a (w < q,
// ws = floor(w 2^64 / q), q < 2^62).  rk = r(k); k <= a fits 64 bits, but qh + 1 is never formed (a faulted qh may be 2^64 - 1).
FHE_HD u64 bc_shoup_k(u64 a, u64 w, u64 ws, u64 q, u32 &rk, const PwFault &f, bool first, bool closing)
{
    const u64 lo = first ? pw_hit(a * w, f, PW_AT_PRODUCT) : a * w;
    const u64 qh = closing ? pw_hit(mulhi64(a, ws), f, PW_AT_QUOTIENT) : mulhi64(a, ws);
    const u64 r = lo - qh * q;
    const bool s = r >= q;
    rk = res_add(res64(qh), (u32)s);
    return s ? r - q : r;
}

// One mixed-radix digit.  raw = input word of limb j (any 64-bit word: the Shoup product folds it, as the unchecked kernels
// do; a word >= p raises PW_OPERAND alone); c[l], rc[l] = r(c[l]) for l < j the earlier digits as they were stored;
// cw(l) = {D_lj, D_lj'} for l < j and cw(j) = {A_j, A_j'}; rp = r(p).  Returns the digit, flags = its flag bits.
// UNR: unroll count of the term loop (the kernels with a compile-time m pass m, so that c[] and rc[] stay in registers)
template <int UNR = 1, class CW>
FHE_HD u64 bc_checked_digit(u64 raw, int j, const u64 *c, const u32 *rc, CW cw, u64 p, u32 rp, u32 &flags, const PwFault &f)
{
    const Tw a = cw(j);
    u32 rk;
    u64 t = bc_shoup_k(raw, a.a, a.b, p, rk, f, true, j == 0);
    u32 rhs = res_mul(res64(raw), res64(a.a)), rK = rk;
#pragma unroll UNR
    for (int l = 0; l < j; l++) {
        const Tw w = cw(l);
        const u64 u = bc_shoup_k(c[l], w.a, w.b, p, rk, f, false, l == j - 1);
        rhs = res_sub(rhs, res_mul(rc[l], res64(w.a)));
        u64 s = t - u;                                        // both below 2^62: the sign is bit 63
        if (l == j - 1) s = pw_hit(s, f, PW_AT_SUM);
        const bool neg = (long long)s < 0;
        t = neg ? s + p : s;
        rK = res_sub(rK, res_add(rk, (u32)neg));              // + p on the value is - 1 on K
    }
    // A digit that is n p too high with K n too low (a closing quotient that came out too small) is consistent: the next digit
    // would come out n lower and every output the same.  Inside the running sum's own window (n < 64, the largest number of
    // terms) it is folded back here, quotient tracked, so that such a digit is flagged exactly when it is wrong modulo p --
    // which is when the outputs change.  Never taken on a clean run.  Anything further out is left to the window d < p: that
    // is what a wrapped subtraction leaves, and a wrap by a multiple of 2^32 - 1 words (2^b p / 2^64 for some bits b of a
    // quotient and primes just below a power of two) passes the identity, so the window is the only check that sees it.
    if (__builtin_expect(t >= p && (long long)t >= 0, 0)) {
        const u64 n = t / p;
        if (n < 64) {
            t -= n * p;
            rK = res_add(rK, (u32)n);
        }
    }
    const u64 d = pw_hit(t, f, PW_AT_RESULT);
    const u32 lhs = res_add(res64(d), res_mul(rK, rp));
    flags = raw >= p ? (u32)PW_OPERAND : (res_eq(lhs, rhs) ? 0u : (u32)PW_RESIDUE) | (d < p ? 0u : (u32)PW_RANGE);
    return d;
}

// One output of the exact conversion from the m digits (any 64-bit words: a faulted digit is folded by the Shoup product);
// cw(l) = {E_lo, E_lo'}; rq = r(q).
template <int UNR = 1, class CW>
FHE_HD u64 bc_checked_out(int m, const u64 *c, const u32 *rc, CW cw, u64 q, u32 rq, u32 &flags, const PwFault &f)
{
    const Tw e0 = cw(0);
    u32 rk;
    u64 acc = bc_shoup_k(c[0], e0.a, e0.b, q, rk, f, true, m == 1);
    u32 rhs = res_mul(rc[0], res64(e0.a)), rK = rk;
#pragma unroll UNR
    for (int l = 1; l < m; l++) {
        const Tw w = cw(l);
        const u64 u = bc_shoup_k(c[l], w.a, w.b, q, rk, f, false, l == m - 1);
        rhs = res_add(rhs, res_mul(rc[l], res64(w.a)));
        u64 s = acc + u;
        if (l == m - 1) s = pw_hit(s, f, PW_AT_SUM);
        const bool ge = s >= q;
        acc = ge ? s - q : s;
        rK = res_add(rK, res_add(rk, (u32)ge));
    }
    const u64 o = pw_hit(acc, f, PW_AT_RESULT);
    const u32 lhs = res_add(res64(o), res_mul(rK, rq));
    flags = (res_eq(lhs, rhs) ? 0u : (u32)PW_RESIDUE) | (o < q ? 0u : (u32)PW_RANGE);
    return o;
}

// One output of the fast conversion: the unreduced sum of the m reduced terms (k_bconv_fast).  x(j) = input word of limb j
// (any 64-bit word, never PW_OPERAND: the Shoup quotient of a 64-bit word fits 64 bits); cw(j) = {C_jo, C_jo'};
// bound = m q (below 2^64 on every plan the fast call accepts).  The word is not canonical, so the identity alone would pass a
// term that is off by a multiple of q (a quotient one too low that the single conditional subtraction cannot absorb): every
// reduced term has its own window t < q next to the word's window below m q.
template <class CX, class CW>
FHE_HD u64 bc_checked_fast(int m, CX x, CW cw, u64 q, u32 rq, u64 bound, u32 &flags, const PwFault &f)
{
    u64 total = 0;
    u32 rhs = 0, rK = 0;
    bool win = true;
    for (int j = 0; j < m; j++) {
        const u64 xj = x(j);
        const Tw w = cw(j);
        u32 rk;
        const u64 u = bc_shoup_k(xj, w.a, w.b, q, rk, f, j == 0, j == 0);
        if (j >= 1 && j == m - 1) total = pw_hit(total, f, PW_AT_SUM);
        total += u;
        win = win && u < q;
        rhs = res_add(rhs, res_mul(res64(xj), res64(w.a)));
        rK = res_add(rK, rk);
    }
    const u64 o = pw_hit(total, f, PW_AT_RESULT);
    const u32 lhs = res_add(res64(o), res_mul(rK, rq));
    flags = (res_eq(lhs, rhs) ? 0u : (u32)PW_RESIDUE) | (win && o < bound ? 0u : (u32)PW_RANGE);
    return o;
}

// which injection points exist on a unit with `terms` terms
FHE_HD bool bc_point_exists(int point, int terms) { return point >= 0 && point <= 3 && (point != PW_AT_SUM || terms >= 2); }

} // namespace fhe
