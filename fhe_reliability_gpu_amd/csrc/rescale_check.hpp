// rescale_check.hpp -- residue-checked form of the one rescale stage that had none: the residues of the dropped limb modulo
// every remaining prime (host + device: the kernel of rescale_checked.hip and the CPU emulation in
// tests/emu/emu_rescale_check.cpp compile the same function).
//
// A rescale takes x = [c]_{q_last} in coefficient form, 0 <= x < q_last, and needs delta_j = x mod q_j for every j < L - 1.  The
// unchecked routes form it on a load (the residues' column pass, ntt_core.hpp) or as a one-limb conversion; both yield the
// canonical residue, which is unique.  The element below forms it as barrett128(x, 0, q_j) of modarith.hpp restated with its
// quotient,
//     x = k q_j + delta_j,      0 <= delta_j < q_j,
// and checks that identity modulo m = 2^32 - 1 with the 32-bit lane arithmetic of residue_check.hpp, which shares nothing with
// the 64-bit multiplies that made k and delta_j:
//     r(delta_j) + r(k) r(q_j)  ==  r(x)   (mod m)
// together with two windows: delta_j < q_j, and the quotient estimate qhat <= x >> floor(log2 q_j) (an upper bound of x / q_j).
//
// Coverage: a single-bit flip of the stored word moves the left side by +-2^b, never 0 modulo m.  A flip of the quotient
// estimate by 2^b that the two conditional subtractions absorb (one or two too low) gives the right word with the right k and
// raises nothing.  Any other change of the quotient moves the remainder by a multiple of q_j: modulo m that is visible unless
// the change of k is a multiple of m / gcd(q_j, m) (gcd > 1 only for the primes 3, 5, 17, 257, 65537), or the 64-bit remainder
// wrapped by a multiple of m words (2^b q_j = t m 2^64 + small, which primes just below a power of two allow: 2^46 (2^50 - 2^18
// + 1) = m 2^64 + 2^46).  Both are left to the windows: with qhat inside its window, qhat q_j < 2 x < 2^62, so the remainder
// x - qhat q_j is either the right one plus at most 2 q_j (absorbed) or outside [0, 3 q_j) and the word fails delta_j < q_j; with
// qhat outside its window the word is flagged whatever it is -- and it is then never the right word, because the right word
// needs the right k.  So a flag is raised exactly when the stored word differs from the clean one.
// Not covered: faults already in x (the checked INTT before this stage answers for it), a register fault on x before both the
// Barrett step and r(x) have read it, faults in the limb constants.  x >= q_last is not a residue of the dropped prime: its
// words are still barrett128's (x mod q_j for any 64-bit x) but cannot be vouched for: PW_OPERAND alone.
//
// Injection points (residue_check.hpp PW_AT_*): PRODUCT = the high word of x * ratio_hi, the product that forms the quotient
// estimate; QUOTIENT = the estimate itself; RESULT = the word before its window check.  There is no running sum: no SUM point.
#pragma once
#include "residue_check.hpp"

namespace fhe {

// rx = r(x), rq = r(q): the caller folds them once per word / per limb
FHE_HD u64 checked_reduce_word(u64 x, u64 qlast, u64 q, u64 r0, u64 r1, u32 rx, u32 rq, u32 &flags, const PwFault &f)
{
    // barrett128(x, 0, q, r0, r1): the terms with hi vanish
    const u64 c = mulhi64(x, r0);
    const u64 t1l = x * r1, t1h = pw_hit(mulhi64(x, r1), f, PW_AT_PRODUCT);
    const u64 s = t1l + c;
    const u64 qhat = pw_hit(t1h + (u64)(s < t1l), f, PW_AT_QUOTIENT);
    u64 r = x - qhat * q;
    const bool s1 = r >= q;
    r = s1 ? r - q : r;
    const bool s2 = r >= q;
    r = s2 ? r - q : r;
    const u64 d = pw_hit(r, f, PW_AT_RESULT);
    const u32 rk = res_add(res64(qhat), (u32)s1 + (u32)s2);      // qhat + 2 is never formed (a faulted qhat may be 2^64 - 1)
    const u32 lhs = res_add(res64(d), res_mul(rk, rq));
    const bool win = d < q && qhat <= (x >> (63 - __builtin_clzll(q)));
    flags = x >= qlast ? (u32)PW_OPERAND : (res_eq(lhs, rx) ? 0u : (u32)PW_RESIDUE) | (win ? 0u : (u32)PW_RANGE);
    return d;
}

// which injection points exist: no running sum
FHE_HD bool rescale_reduce_point_exists(int point) { return point >= 0 && point <= 2; }

} // namespace fhe
