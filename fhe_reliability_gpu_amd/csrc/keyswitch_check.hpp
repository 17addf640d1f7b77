// keyswitch_check.hpp -- residue-checked forms of the two key-switch stages that had none (host + device: the kernels of
// keyswitch_checked.hip and the CPU emulation in tests/emu/emu_keyswitch_check.cpp compile the same functions).
//
// Inner product with the key (MULTEVK, aux_kernels.hip k_ks_mac): per word and key half
//     sum_{d < dnum} x_d y_d = K q + c,      0 <= c < q,
// dnum a run-time count.  KsDotU64 / KsDotF64 restate KsMacU64 / KsMacF64 term by term, including the fold of the running
// sum after every eighth term ((term & 7) == 7: barrett128 / ArithF64::reduce), so that the words are k_ks_mac's bit for bit,
// and carry next to the sum the residue modulo m = 2^32 - 1 of the total quotient K = sum of the folds' quotients (+ the FP64
// terms' own quotients).  K itself can pass 64 bits on the integer path (up to eight folds of quotients near 2^64) and 2^53 on
// the FP64 path (64 terms of quotients near 2^50): only its residue is kept (the rule of baseconv_check.hpp); the FP64 path
// sums the quotients of at most eight terms and one fold in a double (below 2^53: exact) and converts once per fold.  Checked:
//     r(c) + r(K) r(q)  ==  sum_d r(x_d) r(y_d)   (mod m)
// with 32-bit lane arithmetic (residue_check.hpp res_*) that shares nothing with the 64-bit multiplies which made c, and the
// windows: c < q; FP64: the running sum before EVERY fold and before the final reduction |s| < min(dnum, 8) q (a fold would
// otherwise bring a sum that a flipped exponent bit scaled by 2^32 = 1 (mod m) back into range unseen), the value after the
// final reduction in [0, q), every quotient partial finite and below 2^62.
//
// Mod-down tail (aux_kernels.hip k_sub_scale, the arithmetic that also rides on k_ntt_row_subscale):
//     out = ((x - y mod q) s mod q + add) mod q,        (x - y) s + add = K q + out,   K signed
// with d = x - y + b q (b = the borrow), d s = k1 q + v (barrett128), v + add = out + e q (e = the conditional subtraction):
// K = k1 - b s + e.  Checked:  r(out) + r(K) r(q) == (r(x) - r(y)) r(s) + r(add)  (mod m), and the window out < q.
//
// Coverage (both): a single-bit flip of a product word, a running sum, a quotient or the stored word moves one side of the
// identity by +-2^j (times q for a quotient), never 0 modulo m because m is odd and gcd(q, m) = 1 for every prime but 3, 5,
// 17, 257, 65537 -- for those a change of K by a multiple of m / q is left to the window (a single-bit flip of K is never one).
// A quotient flip that wraps the 64-bit remainder leaves a word outside [0, q): the window sees it.  An intermediate that is
// off but consistent (a Barrett estimate one too low that the conditional subtraction absorbs, an FP64 quotient moved by d with
// the value moved by d q and folded back) gives the right word and raises nothing.  Not covered: faults already in the
// operands, a register fault on an operand before both the product and its residue have read it.  Operands that are not
// canonical (>= q) are folded as the unchecked kernels fold them but cannot be checked: the element raises PW_OPERAND alone and
// its word is still the unchecked kernel's.
//
// Injection points (residue_check.hpp PW_AT_*): PRODUCT = the first term's product before reduction (U64: low word of the
// 128-bit product; FP64: h; tail: low word of d s); QUOTIENT = the quotient estimate of the reduction that produces the word
// (the final one, not a fold's; tail: the Barrett step of d s); RESULT = the word before its window check; SUM = the running
// sum before its final reduction (tail: v + add before the conditional subtraction -- exists only with an addend).
#pragma once
#include "residue_check.hpp"
#include "baseconv_check.hpp"

namespace fhe {

// ---- inner product, U64 path (KsMacU64) ----
struct KsDotU64 {
    u64 lo = 0, hi = 0;
    u32 rhs = 0, rK = 0;
    bool canon = true;
    FHE_HD void mac(u64 x, u64 y, u32 term, const LimbParams &p, const PwFault &f)
    {
        canon = canon && x < p.q && y < p.q;
        const u64 a = x < p.q ? x : reduce_any_u64(x, p.q);
        const u64 b = y < p.q ? y : reduce_any_u64(y, p.q);
        const u64 pl = term == 0 ? pw_hit(a * b, f, PW_AT_PRODUCT) : a * b, ph = mulhi64(a, b);      // < 2^124
        lo += pl;
        hi += ph + (lo < pl);
        rhs = res_add(rhs, res_mul(res64(a), res64(b)));
        if ((term & 7) == 7) {
            u64 k;
            lo = barrett128_k(lo, hi, p.q, p.barrett_lo, p.barrett_hi, k, PwFault{-1, 0});
            hi = 0;
            rK = res_add(rK, res64(k));
        }
    }
    FHE_HD u64 finish(u32, const LimbParams &p, u32 &flags, const PwFault &f)
    {
        u64 k;
        const u64 c = pw_hit(barrett128_k(pw_hit(lo, f, PW_AT_SUM), hi, p.q, p.barrett_lo, p.barrett_hi, k, f), f, PW_AT_RESULT);
        const u32 lhs = res_add(res64(c), res_mul(res_add(rK, res64(k)), res64(p.q)));
        flags = !canon ? (u32)PW_OPERAND : (res_eq(lhs, rhs) ? 0u : (u32)PW_RESIDUE) | (c < p.q ? 0u : (u32)PW_RANGE);
        return c;
    }
};

// ---- inner product, FP64 path (KsMacF64, q < 2^50) ----
struct KsDotF64 {
    double s = 0.0, kp = 0.0;      // running sum; quotients since the last fold (at most eight terms and one fold: below 2^53)
    u32 rhs = 0, rK = 0;
    bool canon = true, win = true;
    // r(kp) into rK; a partial that is not a finite integer below 2^62 fails the window
    FHE_HD void fold_quotients(double extra)
    {
        const double kt = __builtin_rint(kp + extra);
        const bool ok = __builtin_fabs(kt) < 0x1p62;      // false for NaN
        win = win && ok;
        rK = res_add(rK, res_i64(ok ? (long long)kt : 0));
        kp = 0.0;
    }
    FHE_HD void mac(u64 x, u64 y, u32 term, const LimbParams &p, const PwFault &f)
    {
        const ArithF64::Ctx c = ArithF64::make_ctx(p);
        canon = canon && x < p.q && y < p.q;
        const u64 xr = x < p.q ? x : reduce_any_u64(x, p.q), yr = y < p.q ? y : reduce_any_u64(y, p.q);
        const double a = ArithF64::from_canonical(xr), b = ArithF64::from_canonical(yr);
        const double h = a * b;
        const double k = __builtin_rint(a * (b * c.ninv));
        const double l = __builtin_fma(a, b, -h);
        s += __builtin_fma(-k, c.n, term == 0 ? pw_hit(h, f, PW_AT_PRODUCT) : h) + l;          // |term| < 0.875 q
        kp += k;
        rhs = res_add(rhs, res_mul(res64(xr), res64(yr)));
        if ((term & 7) == 7) {
            win = win && __builtin_fabs(s) < 8.0 * c.n;       // 0.5 q left by the last fold + eight terms
            const double kf = __builtin_rint(s * c.ninv);     // ArithF64::reduce, with its quotient
            s = __builtin_fma(-kf, c.n, s);
            fold_quotients(kf);
        }
    }
    FHE_HD u64 finish(u32 terms, const LimbParams &p, u32 &flags, const PwFault &f)
    {
        const ArithF64::Ctx c = ArithF64::make_ctx(p);
        s = pw_hit(s, f, PW_AT_SUM);
        const double k = pw_hit(__builtin_rint(s * c.ninv), f, PW_AT_QUOTIENT);
        double v = __builtin_fma(-k, c.n, s);
        const bool neg = v < 0.0;
        if (neg) v += c.n;
        const u64 w = pw_hit(ArithF64::to_u64(v), f, PW_AT_RESULT);
        fold_quotients(k - (neg ? 1.0 : 0.0));
        const double bound = (terms < 8 ? (double)terms : 8.0) * c.n;
        const bool ok = win && __builtin_fabs(s) < bound && v >= 0.0 && v < c.n && w < p.q;
        const u32 lhs = res_add(res64(w), res_mul(rK, res64(p.q)));
        flags = !canon ? (u32)PW_OPERAND : (res_eq(lhs, rhs) ? 0u : (u32)PW_RESIDUE) | (ok ? 0u : (u32)PW_RANGE);
        return w;
    }
};

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
