// scalar_check.hpp -- residue-checked form of the word-wise scalar multiply / affine map c = a s + o mod q (aux_kernels.hip
// k_scalar_affine), the step the BGV forms of the key switch and of the mod switch put between their transforms and conversions
// (times t^-1 on the limbs about to be converted, times t on the converted ones).  Host + device: the kernel of scalar_checked.hip
// and the CPU emulation in tests/emu/emu_scalar_check.cpp compile the same function.
//
// The element restates k_scalar_affine -- mulmod_b(a, s), plus o, one conditional subtraction -- with barrett128_k of
// residue_check.hpp, the Barrett step checked_modmul_barrett is made of, so that the words are the unchecked kernel's bit for bit
// for any 64-bit a, and tracks the quotient next to it:
//     a s (+ o) = k q + c,      0 <= c < q,      k = the Barrett estimate + the conditional subtractions taken
// for canonical a, s, o.  Checked modulo m = 2^32 - 1 with the 32-bit lane arithmetic of residue_check.hpp, which shares nothing
// with the 64-bit multiplies that made k and c:
//     r(c) + r(k) r(q)  ==  r(a) r(s) (+ r(o))   (mod m)
// together with two windows: c < q, and the quotient within 2^24 of the FP64 estimate a s / q.
//
// Why the second window.  A wrong quotient k + d leaves the 64-bit remainder c - d q + t 2^64 for some integer t, and the identity
// then fails by t modulo m (2^64 = 1).  t = 0: the remainder is off by d q exactly and the first window sees it unless the two
// conditional subtractions absorb it (an estimate one or two too low: the right word with the right k, nothing raised).  0 < |t|
// < m: the identity sees it.  |t| >= m needs |d| q >= m 2^64 - 3 q, |d| > 2^34 for q < 2^61 -- and then the word can pass both
// other checks: 2^46 (2^50 - 2^18 + 1) = m 2^64 + 2^46 leaves c - 2^46, inside [0, q) whenever c >= 2^46.  A product's quotient
// is as large as a, so no bound of the kind the rescale's residues use (x >> floor(log2 q)) separates k + 2^46 from k; the FP64
// estimate does: three roundings on a value below 2^61 keep it within 2^10 of k.  It is made from a, s and 1 / q by the FP64
// pipe and shares no instruction with the integer multiplies.  A quotient outside this window never gives the right word (d q = t
// 2^64 + (0, 1 or 2) q has no solution with 0 < |d| < 2^64 for odd q), so a flag is raised exactly when the stored word differs
// from the clean one.
// Not covered: faults already in a (the stage before answers for it), a register fault on a before the product, its residue and
// the estimate have all read it, faults in the limb constants or the scalars.  a >= q (or a scalar that the caller did not
// reduce) cannot be checked -- the quotient can pass 64 bits --: PW_OPERAND alone, the word still k_scalar_affine's.
//
// Injection points (residue_check.hpp PW_AT_*): PRODUCT = the low word of the 128-bit product a s, QUOTIENT = the Barrett
// estimate, RESULT = the word before its window check, SUM (ADD only) = a s mod q + o before the conditional subtraction.
#pragma once
#include "residue_check.hpp"

namespace fhe {

// ADD: with the addend o (without, o is not read and SUM does not exist).  rq = r(q), ninv = 1.0 / q (LimbParams::ninv)
template <bool ADD>
FHE_HD u64 checked_scalar_affine(u64 a, u64 s, u64 o, u64 q, u64 r0, u64 r1, double ninv, u32 rq, u32 &flags, const PwFault &f)
{
    u64 k;
    u64 c = barrett128_k(pw_hit(a * s, f, PW_AT_PRODUCT), mulhi64(a, s), q, r0, r1, k, f);
    u32 rhs = res_mul(res64(a), res64(s));
    bool canon = a < q && s < q;
    if (ADD) {
        const u64 v = pw_hit(c + o, f, PW_AT_SUM);      // k_scalar_affine adds the scalar as it is: the caller reduced it
        const bool sub = v >= q;
        c = sub ? v - q : v;
        k += (u64)sub;
        rhs = res_add(rhs, res64(o));
        canon = canon && o < q;
    }
    c = pw_hit(c, f, PW_AT_RESULT);
    const u32 lhs = res_add(res64(c), res_mul(res64(k), rq));
    const double est = (double)a * (double)s * ninv;
    const bool win = c < q && __builtin_fabs((double)k - est) < 0x1p24;
    flags = !canon ? (u32)PW_OPERAND : (res_eq(lhs, rhs) ? 0u : (u32)PW_RESIDUE) | (win ? 0u : (u32)PW_RANGE);
    return c;
}

// which injection points exist: the running sum only with an addend
FHE_HD bool scalar_affine_point_exists(int point, bool has_add) { return point >= 0 && (point <= 2 || (point == 3 && has_add)); }

} // namespace fhe
