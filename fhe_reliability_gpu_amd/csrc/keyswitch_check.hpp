// keyswitch_check.hpp -- residue-checked forms of the two key-switch stages that had none (host + device: the kernels of
// keyswitch_checked.hip and the CPU emulation in tests/emu/emu_keyswitch_check.cpp compile the same functions).
//
// Inner product with the key (MULTEVK, aux_kernels.hip k_ks_mac): per word and key half
//     sum_{d < dnum} x_d y_d = K q + c,      0 <= c < q,
// dnum a run-time count: KsDotU64 / KsDotF64 of residue_check.hpp, which states the eight-term fold, the identity, the
// windows, the coverage and the injection points.
//
// Mod-down tail (aux_kernels.hip k_sub_scale, the arithmetic that also rides on k_ntt_row_subscale):
//     out = ((x - y mod q) s mod q + add) mod q,        (x - y) s + add = K q + out,   K signed
// with d = x - y + b q (b = the borrow), d s = k1 q + v (barrett128), v + add = out + e q (e = the conditional subtraction):
// K = k1 - b s + e.  Checked with the res_* lane arithmetic:  r(out) + r(K) r(q) == (r(x) - r(y)) r(s) + r(add)  (mod m), and
// the window out < q.  Coverage and the rule for operands >= q (PW_OPERAND alone, the word still the unchecked kernel's) are
// those of residue_check.hpp.  Injection points (PW_AT_*): PRODUCT = the low word of d s; QUOTIENT = the Barrett step of d s;
// RESULT = the word before its window check; SUM = v + add before the conditional subtraction -- exists only with an addend.
#pragma once
#include "residue_check.hpp"
#include "baseconv_check.hpp"

namespace fhe {

// ---- mod-down tail element (k_sub_scale): out = ((x - y mod q) s mod q + add) mod q; has_x / has_y / has_add = the operand
// exists (an absent one is zero, as SubScaleArgs' null pointers); s < q is the plan's constant P^-1 mod q ----
FHE_HD u64 checked_sub_scale(u64 xa, bool has_x, u64 ya, bool has_y, u64 s, u64 adda, bool has_add, u64 q, u64 r0, u64 r1, u32 rq, u32 &flags,
                             const PwFault &f)
{
    const bool canon = (!has_x || xa < q) && (!has_y || ya < q) && (!has_add || adda < q);
    const u64 x = has_x ? barrett128(xa, 0, q, r0, r1) : 0, y = has_y ? barrett128(ya, 0, q, r0, r1) : 0;      // the word itself when canonical
    const bool borrow = x < y;
    const u64 d = borrow ? x + q - y : x - y;
    u64 k1;
    u64 v = barrett128_k(pw_hit(d * s, f, PW_AT_PRODUCT), mulhi64(d, s), q, r0, r1, k1, f);
    const u32 rs = res64(s);
    u32 rK = res64(k1), rhs = res_mul(res_sub(res64(x), res64(y)), rs);
    if (borrow) rK = res_sub(rK, rs);            // d = x - y + q: - s on K
    if (has_add) {
        const u64 ad = barrett128(adda, 0, q, r0, r1);
        v = pw_hit(v + ad, f, PW_AT_SUM);
        const bool sub = v >= q;
        v = sub ? v - q : v;
        rK = res_add(rK, (u32)sub);
        rhs = res_add(rhs, res64(ad));
    }
    v = pw_hit(v, f, PW_AT_RESULT);
    const u32 lhs = res_add(res64(v), res_mul(rK, rq));
    flags = !canon ? (u32)PW_OPERAND : (res_eq(lhs, rhs) ? 0u : (u32)PW_RESIDUE) | (v < q ? 0u : (u32)PW_RANGE);
    return v;
}

// which injection points exist: the tail's running sum only with an addend
FHE_HD bool ks_tail_point_exists(int point, bool has_add) { return point >= 0 && point <= 3 && (point != PW_AT_SUM || has_add); }

} // namespace fhe
