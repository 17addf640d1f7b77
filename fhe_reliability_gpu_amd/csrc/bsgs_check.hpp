// bsgs_check.hpp -- residue-checked forms of the two kernels of the BSGS matrix-vector product that had none (host + device: the
// kernels of bsgs_checked.hip and the CPU emulation in tests/emu/emu_bsgs_check.cpp compile the same functions).
//
// Inner sum (aux_kernels.hip k_diag_mac): per word and ciphertext part h
//     sum_{b < n1} d_b y_b,h = K_h q + c_h,      0 <= c_h < q,
// d_b the diagonal word shared by both parts, y_b,h the word of part h of the b-th rotated ciphertext, n1 a run-time count.
// k_diag_mac accumulates with KsMacU64 / KsMacF64 and the term index b, so the running sums are folded after every eighth term:
// KsDotU64 / KsDotF64 of keyswitch_check.hpp restate exactly that recurrence term by term and carry the residue of the total
// quotient.  DiagDot runs two of them, one per part, over the same diagonal word (the diagonal is the FIRST operand, as in
// k_diag_mac: the FP64 quotient estimate a (b / q) is not symmetric).  Checked per part, with the windows those structs apply:
//     r(c_h) + r(K_h) r(q)  ==  sum_b r(d_b) r(y_b,h)   (mod m = 2^32 - 1)
// A diagonal word >= q is folded as the unchecked kernel folds it and raises PW_OPERAND alone on BOTH parts; a word of one part
// that is >= q raises it on that part only.  Injection points (residue_check.hpp PW_AT_*) with their meaning in keyswitch_check.hpp:
// PRODUCT = the first term's product, QUOTIENT = the final reduction's quotient estimate, RESULT = the word before its window
// check, SUM = the running sum before its final reduction; each part has its own PwFault, so the hook names the part it hits.
//
// Add (aux_kernels.hip k_modadd): c = a + b - e q, e in {0, 1}, both operands reduced with barrett128 first (the word itself when
// canonical).  Checked:  r(c) + e r(q) == r(a) + r(b)  (mod m)  and the window c < q.  Operands >= q are folded exactly as k_modadd
// folds them but cannot be checked: the element raises PW_OPERAND alone and its word is still k_modadd's.  Injection points:
// SUM = a + b before the conditional subtraction, RESULT = the word before its window check; there is no product and no quotient
// estimate (modadd_point_exists).
//
// Coverage (both): as keyswitch_check.hpp -- a single-bit flip of a product word, a running sum, a quotient or the stored word
// moves one side of the identity by +-2^j (times q for a quotient), never 0 modulo the odd m.  A flip of a + b changes the word
// whatever the subtraction then does (2^j is never a multiple of q) and moves the left side alone.  Not covered: faults already
// in the operands, a register fault on an operand before both the arithmetic and its residue have read it.
#pragma once
#include "keyswitch_check.hpp"

namespace fhe {

// ---- inner sum: D = KsDotU64 or KsDotF64, one accumulator per ciphertext part over the same diagonal word ----
template <class D> struct DiagDot {
    D s0, s1;
    FHE_HD void mac(u64 d, u64 y0, u64 y1, u32 b, const LimbParams &p, const PwFault &f0, const PwFault &f1)
    {
        s0.mac(d, y0, b, p, f0);
        s1.mac(d, y1, b, p, f1);
    }
    FHE_HD void finish(u32 n1, const LimbParams &p, u64 &c0, u64 &c1, u32 &fl0, u32 &fl1, const PwFault &f0, const PwFault &f1)
    {
        c0 = s0.finish(n1, p, fl0, f0);
        c1 = s1.finish(n1, p, fl1, f1);
    }
};

// ---- add element (k_modadd): c = (a + b) mod q for any 64-bit words; rq = r(q) ----
FHE_HD u64 checked_modadd(u64 aa, u64 ba, u64 q, u64 r0, u64 r1, u32 rq, u32 &flags, const PwFault &f)
{
    const bool canon = aa < q && ba < q;
    const u64 a = barrett128(aa, 0, q, r0, r1), b = barrett128(ba, 0, q, r0, r1);      // the word itself when canonical
    const u64 s = pw_hit(a + b, f, PW_AT_SUM);                                           // < 2^62: no carry
    const bool sub = s >= q;
    const u64 c = pw_hit(sub ? s - q : s, f, PW_AT_RESULT);
    const u32 lhs = res_add(res64(c), sub ? rq : 0u), rhs = res_add(res64(a), res64(b));
    flags = !canon ? (u32)PW_OPERAND : (res_eq(lhs, rhs) ? 0u : (u32)PW_RESIDUE) | (c < q ? 0u : (u32)PW_RANGE);
    return c;
}

// which injection points exist on the add: the sum and the result
FHE_HD bool modadd_point_exists(int point) { return point == PW_AT_RESULT || point == PW_AT_SUM; }

} // namespace fhe
