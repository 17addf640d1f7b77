// residue_check.hpp -- residue-checked element-wise modular products (host + device: the kernels of pointwise_checked.hip and
// the CPU emulation in tests/emu/emu_pointwise.cpp compile the same functions).
//
// Every product kernel forms an integer quotient k and a word c with
//     sum_t a_t b_t (+ o, the old word when accumulating) = k q + c,      0 <= c < q
// for canonical operands.  The functions below restate that arithmetic -- barrett128 of modarith.hpp for k_modmul and
// KsMacU64, the FMA term h - k q + l and ArithF64::canonical for KsMacF64 -- so that they produce the very same words, and
// track k next to it.  The identity is then checked modulo m = 2^32 - 1 with 32-bit lane arithmetic that shares nothing with
// the 64-bit multiply which made c:
//     r(c) + r(k) r(q)  ==  sum_t r(a_t) r(b_t) (+ r(o))   (mod m),      r(x) = x mod m, folded from the 32-bit halves of x
// together with the window c < q.  For Barrett, the pre-subtraction window (lo - qhat q < 3q) is the same compare: the two
// conditional subtractions leave c < q exactly when it holds.  An intermediate that is out of its window but consistent (the
// Barrett remainder before an accumulate, an FP64 quotient shifted by d with the value shifted by d q) gives the right word
// and raises nothing.  This one identity does the work of the reference's Intra (fold residue of a, b and the product) and
// Sum (reduced against unreduced sum) checks of rfhe_framewk/src/barrett_final.py.
//
// Coverage: a single-bit error in the product, the quotient or c changes one side by +-2^j, and 2^j is never 0 mod m; since
// gcd(q, m) = 1 for every prime but the five factors of m (3, 5, 17, 257, 65537), any change of k is caught as well -- for
// those five primes a change of k by a multiple of m / q is left to the window (a single-bit flip of k is never one).  Not
// covered: faults already in the operands, and a register fault on a or b before both the product and its residue have
// read it.  Operands that are not canonical (a, b or o >= q) cannot be checked (the
// quotient can exceed 64 bits): their element raises PW_OPERAND alone, and its word is still the unchecked call's.
#pragma once
#include "modarith.hpp"

namespace fhe {

enum { PW_RESIDUE = 1, PW_RANGE = 2, PW_OPERAND = 4 };      // flag bits
// injection points of the test hook: the product before reduction (U64: low word of the 128-bit product, FP64: h), the
// quotient estimate of the reduction that produces the word, the word before its range check, the running sum before
// its final reduction
enum { PW_AT_PRODUCT = 0, PW_AT_QUOTIENT = 1, PW_AT_RESULT = 2, PW_AT_SUM = 3 };
struct PwFault {
    int point;      // < 0: none
    u64 mask;       // XORed into the value at `point` (0 for every element but the target)
};
FHE_HD u64 pw_hit(u64 v, const PwFault &f, int at) { return f.point == at ? v ^ f.mask : v; }
FHE_HD double pw_hit(double v, const PwFault &f, int at) { return f.point == at ? u64_bits_to_double(double_to_u64_bits(v) ^ f.mask) : v; }

// ---- arithmetic modulo m = 2^32 - 1 (one's complement: 0 and 0xFFFFFFFF both stand for 0) ----
FHE_HD u32 res_add(u32 a, u32 b)
{
    const u32 s = a + b;
    return s + (u32)(s < a);        // end-around carry: 2^32 = 1 (mod m)
}
FHE_HD u32 res64(u64 x) { return res_add((u32)x, (u32)(x >> 32)); }
FHE_HD u32 res_mul(u32 a, u32 b) { return res64((u64)a * b); }
// a signed quotient: (u64)k = k + 2^64 = k + 1 (mod m) for k < 0
FHE_HD u32 res_i64(long long k) { return k < 0 ? res_add(res64((u64)k), 0xFFFFFFFEu) : res64((u64)k); }
FHE_HD bool res_eq(u32 a, u32 b) { return (a == 0xFFFFFFFFu ? 0u : a) == (b == 0xFFFFFFFFu ? 0u : b); }

// barrett128 (modarith.hpp) with its quotient: k = qhat + the conditional subtractions taken
FHE_HD u64 barrett128_k(u64 lo, u64 hi, u64 q, u64 r0, u64 r1, u64 &k, const PwFault &f)
{
    const u64 c = mulhi64(lo, r0);
    const u64 t1l = lo * r1, t1h = mulhi64(lo, r1);
    const u64 t2l = hi * r0, t2h = mulhi64(hi, r0);
    u64 s = t1l + t2l;
    u64 carry = s < t1l;
    const u64 s2 = s + c;
    carry += s2 < s;
    const u64 qhat = pw_hit(hi * r1 + t1h + t2h + carry, f, PW_AT_QUOTIENT);
    u64 r = lo - qhat * q;
    const bool s1 = r >= q;
    r = s1 ? r - q : r;
    const bool sb = r >= q;
    r = sb ? r - q : r;
    k = qhat + (u64)s1 + (u64)sb;
    return r;
}

// Barrett form: k_modmul's element, c = a b mod q, or (ACC) c = (o + a b) mod q with o the old word, for any 64-bit words
// (aux_kernels.hip mulmod_b + the accumulate).  rq = r(q).  Returns the word; *flags = its flag bits.
template <bool ACC>
FHE_HD u64 checked_modmul_barrett(u64 a, u64 b, u64 o, u64 q, u64 r0, u64 r1, u32 rq, u32 &flags, const PwFault &f)
{
    u64 k;
    u64 c = barrett128_k(pw_hit(a * b, f, PW_AT_PRODUCT), mulhi64(a, b), q, r0, r1, k, f);
    u32 rhs = res_mul(res64(a), res64(b));
    bool canon = a < q && b < q;
    if (ACC) {
        const u64 s = pw_hit(c + (o < q ? o : barrett128(o, 0, q, r0, r1)), f, PW_AT_SUM);   // barrett128(o, 0) = o for o < q
        const bool sub = s >= q;
        c = sub ? s - q : s;
        k += (u64)sub;
        rhs = res_add(rhs, res64(o));
        canon = canon && o < q;
    }
    c = pw_hit(c, f, PW_AT_RESULT);
    const u32 lhs = res_add(res64(c), res_mul(res64(k), rq));
    flags = !canon ? (u32)PW_OPERAND : (res_eq(lhs, rhs) ? 0u : (u32)PW_RESIDUE) | (c < q ? 0u : (u32)PW_RANGE);
    return c;
}

// U64 sum of T products (KsMacU64 of aux_kernels.hip for T <= 7 terms: operands reduced first, 128-bit running sum, one
// Barrett step at the end).  The fault at PW_AT_PRODUCT hits the first term.
template <int T>
FHE_HD u64 checked_dot_u64(const u64 (&x)[T], const u64 (&y)[T], const LimbParams &p, u32 &flags, const PwFault &f)
{
    u64 lo = 0, hi = 0;
    u32 rhs = 0;
    bool canon = true;
    for (int t = 0; t < T; t++) {
        canon = canon && x[t] < p.q && y[t] < p.q;
        const u64 a = x[t] < p.q ? x[t] : reduce_any_u64(x[t], p.q);
        const u64 b = y[t] < p.q ? y[t] : reduce_any_u64(y[t], p.q);
        const u64 pl = t == 0 ? pw_hit(a * b, f, PW_AT_PRODUCT) : a * b, ph = mulhi64(a, b);
        lo += pl;
        hi += ph + (lo < pl);
        rhs = res_add(rhs, res_mul(res64(a), res64(b)));
    }
    lo = pw_hit(lo, f, PW_AT_SUM);
    u64 k;
    const u64 c = pw_hit(barrett128_k(lo, hi, p.q, p.barrett_lo, p.barrett_hi, k, f), f, PW_AT_RESULT);
    const u32 lhs = res_add(res64(c), res_mul(res64(k), res64(p.q)));
    flags = !canon ? (u32)PW_OPERAND : (res_eq(lhs, rhs) ? 0u : (u32)PW_RESIDUE) | (c < p.q ? 0u : (u32)PW_RANGE);
    return c;
}

// FP64-term form: the same sum on KsMacF64's arithmetic (q < 2^50).  Each term is h - k q + l with h + l = a b exactly
// (the FMA error-free product), the sum is made canonical by ArithF64::canonical (reduce, then + q when negative); the
// total quotient sum k_t + k_reduce - [+q] is formed in FP64 (exact: integers below 2^53 on a clean run), rounded and
// converted to a signed 64-bit integer.  Windows: the running sum |s| < T q (every term is below 0.875 q), the value after the
// reduction in [0, q), the quotient finite and below 2^62.  The sum window is what catches a flip of an exponent bit that
// scales a value v by 2^32 = 1 (mod m); it misses only when the scaled value stays inside it (2^32 |v| < T q: tiny products).
template <int T>
FHE_HD u64 checked_dot_f64(const u64 (&x)[T], const u64 (&y)[T], const LimbParams &p, u32 &flags, const PwFault &f)
{
    const ArithF64::Ctx c = ArithF64::make_ctx(p);
    double s = 0.0, K = 0.0;
    u32 rhs = 0;
    bool canon = true;
    for (int t = 0; t < T; t++) {
        canon = canon && x[t] < p.q && y[t] < p.q;
        const u64 xr = x[t] < p.q ? x[t] : reduce_any_u64(x[t], p.q), yr = y[t] < p.q ? y[t] : reduce_any_u64(y[t], p.q);
        const double a = ArithF64::from_canonical(xr), b = ArithF64::from_canonical(yr);
        const double h = a * b;
        const double k = __builtin_rint(a * (b * c.ninv));
        const double l = __builtin_fma(a, b, -h);
        s += __builtin_fma(-k, c.n, t == 0 ? pw_hit(h, f, PW_AT_PRODUCT) : h) + l;
        K += k;
        rhs = res_add(rhs, res_mul(res64(xr), res64(yr)));
    }
    s = pw_hit(s, f, PW_AT_SUM);
    const double k = pw_hit(__builtin_rint(s * c.ninv), f, PW_AT_QUOTIENT);
    double v = __builtin_fma(-k, c.n, s);
    const bool neg = v < 0.0;
    if (neg) v += c.n;
    const u64 w = pw_hit(ArithF64::to_u64(v), f, PW_AT_RESULT);
    const double kt = __builtin_rint(K + k) - (neg ? 1.0 : 0.0);
    const bool kok = __builtin_fabs(kt) < 0x1p62;                  // false for NaN
    const bool win = kok && __builtin_fabs(s) < T * c.n && v >= 0.0 && v < c.n && w < p.q;
    const u32 lhs = res_add(res64(w), res_mul(res_i64(kok ? (long long)kt : 0), res64(p.q)));
    flags = !canon ? (u32)PW_OPERAND : (res_eq(lhs, rhs) ? 0u : (u32)PW_RESIDUE) | (win ? 0u : (u32)PW_RANGE);
    return w;
}

} // namespace fhe
