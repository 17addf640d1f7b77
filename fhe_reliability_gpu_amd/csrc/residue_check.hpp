// residue_check.hpp -- residue-checked modular products and sums of products (host + device: the checked kernels and the CPU
// emulations under tests/emu compile the same functions).
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
// Barrett remainder before an accumulate, a Barrett estimate one too low that the conditional subtraction absorbs, an FP64
// quotient shifted by d with the value shifted by d q and folded back) gives the right word and raises nothing.  This one
// identity does the work of the reference's Intra (fold residue of a, b and the product) and Sum (reduced against unreduced
// sum) checks of rfhe_framewk/src/barrett_final.py.
//
// Sums of products (KsDotU64 / KsDotF64: the tensor product's d0, d1, d2 with one or two terms, the key switch's inner
// product and the BSGS inner sum with a run-time count) restate KsMacU64 / KsMacF64 term by term, including the fold of the
// running sum after every eighth term ((term & 7) == 7: barrett128 / ArithF64::reduce), so that the words are the unchecked
// kernels' bit for bit.  The total quotient K = the folds' quotients + the final one (+ the FP64 terms' own) can pass 64 bits
// on the integer path (up to eight folds of quotients near 2^64) and 2^53 on the FP64 path (64 terms of quotients near 2^50):
// only its residue is kept; the FP64 path sums the quotients of at most eight terms and one fold in a double (below 2^53:
// exact) and converts once per fold.  checked_dot_u64<T> / checked_dot_f64<T> are the same structs over T < 8 terms held in
// arrays: the term numbers are constants once the loop is unrolled, so no fold is compiled.
// FP64 windows: the running sum before EVERY fold and before the final reduction |s| < min(terms, 8) q (every term is below
// 0.875 q, a fold leaves 0.5 q), the value after the final reduction in [0, q), every quotient partial finite and below 2^62.
// The sum window is what catches a flip of an exponent bit that scales a value v by 2^32 = 1 (mod m) -- a fold would otherwise
// bring such a sum back into range unseen; it misses only when the scaled value stays inside it (2^32 |v| < terms q: tiny
// products).
//
// Coverage: a single-bit error in a product, a running sum, a quotient or c changes one side by +-2^j (times q for a
// quotient), and 2^j is never 0 mod m; since gcd(q, m) = 1 for every prime but the five factors of m (3, 5, 17, 257, 65537),
// any change of k is caught as well -- for those five primes a change of k by a multiple of m / q is left to the window (a
// single-bit flip of k is never one).  A quotient flip that wraps the 64-bit remainder leaves a word outside [0, q): the
// window sees it.  Not covered: faults already in the operands, and a register fault on a or b before both the product and
// its residue have read it.  Operands that are not canonical (a, b or o >= q) are folded as the unchecked kernels fold them
// but cannot be checked (the quotient can exceed 64 bits): their element raises PW_OPERAND alone, and its word is still the
// unchecked call's.
#pragma once
#include "modarith.hpp"

namespace fhe {

enum { PW_RESIDUE = 1, PW_RANGE = 2, PW_OPERAND = 4 };      // flag bits
// injection points of the test hook: the product before reduction (U64: low word of the 128-bit product, FP64: h; of a sum,
// the first term's), the quotient estimate of the reduction that produces the word (of a sum: the final one, not a fold's),
// the word before its range check, the running sum before its final reduction
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
FHE_HD u32 res_sub(u32 a, u32 b) { return res_add(a, ~b); }      // one's complement: -b = ~b (mod m)
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

// ---- sum of products, U64 path (KsMacU64): mac() the terms 0 .. terms - 1 in order, then finish(terms) ----
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

// ---- sum of products, FP64 path (KsMacF64, q < 2^50): each term is h - k q + l with h + l = a b exactly (the FMA
// error-free product); the sum is made canonical as ArithF64::canonical does (reduce, then + q when negative) ----
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

// T < 8 terms known at compile time on D = KsDotU64 or KsDotF64 (k_tensor_checked: T = 1 and 2)
template <class D, int T>
FHE_HD u64 checked_dot(const u64 (&x)[T], const u64 (&y)[T], const LimbParams &p, u32 &flags, const PwFault &f)
{
    static_assert(T >= 1 && T < 8, "no fold: fewer than eight terms");
    D s;
    for (int t = 0; t < T; t++) s.mac(x[t], y[t], (u32)t, p, f);
    return s.finish((u32)T, p, flags, f);
}
template <int T>
FHE_HD u64 checked_dot_u64(const u64 (&x)[T], const u64 (&y)[T], const LimbParams &p, u32 &flags, const PwFault &f) { return checked_dot<KsDotU64, T>(x, y, p, flags, f); }
template <int T>
FHE_HD u64 checked_dot_f64(const u64 (&x)[T], const u64 (&y)[T], const LimbParams &p, u32 &flags, const PwFault &f) { return checked_dot<KsDotF64, T>(x, y, p, flags, f); }

} // namespace fhe
