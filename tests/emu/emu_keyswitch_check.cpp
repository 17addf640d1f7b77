// emu_keyswitch_check.cpp -- CPU emulation of the checked key-switch inner product and mod-down tail (TEST INFRASTRUCTURE ONLY).
//
// Compiles fhe_reliability_gpu_amd/csrc/keyswitch_check.hpp -- the element functions the kernels of keyswitch_checked.hip
// call -- with g++ and runs them over arrays of elements, with an optional bit flip at one injection point of every
// element, so that words and flag bits can be checked against Python integers without a GPU.  The unchecked elements
// (KsMacU64 / KsMacF64 / k_sub_scale of aux_kernels.hip) are restated here for the operands the checks cannot cover.  The
// library never links this file.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I<csrc> emu_keyswitch_check.cpp -o libemu_keyswitch_check.so
#include "keyswitch_check.hpp"

using namespace fhe;

namespace {

// the limb constants as capi.cpp build_tables fills them (the fields these elements read)
LimbParams limb(u64 q, int path)
{
    LimbParams p{};
    p.q = q;
    p.two_q = 2 * q;
    p.n = (double)q;
    p.ninv = 1.0 / p.n;
    const unsigned __int128 ratio = ~(unsigned __int128)0 / q;      // floor(2^128 / q) for q not a power of two
    p.barrett_lo = (u64)ratio;
    p.barrett_hi = (u64)(ratio >> 64);
    p.path = path;
    return p;
}

PwFault fault(int point, int bit) { return PwFault{point, point < 0 ? 0 : (u64)1 << bit}; }

template <class D>
void dot_checked(const u64 *x, const u64 *y, int terms, size_t n, const LimbParams &p, const PwFault &ft, u64 *w, u32 *f)
{
    for (size_t i = 0; i < n; i++) {
        D s;
        for (int t = 0; t < terms; t++) s.mac(x[(size_t)t * n + i], y[(size_t)t * n + i], (u32)t, p, ft);
        w[i] = s.finish((u32)terms, p, f[i], ft);
    }
}

} // namespace

extern "C" {

// sum of `terms` products per element, x = [terms][n], y = [terms][n]; path 0 = FP64-term form (q < 2^50), 1 = U64
int emu_ks_dot_checked(const u64 *x, const u64 *y, int terms, size_t n, u64 q, int path, int point, int bit, u64 *w, u32 *f)
{
    if (terms < 1 || (path == PATH_F64 && q >= ((u64)1 << 50))) return -1;
    const LimbParams p = limb(q, path);
    if (path == PATH_F64) dot_checked<KsDotF64>(x, y, terms, n, p, fault(point, bit), w, f);
    else dot_checked<KsDotU64>(x, y, terms, n, p, fault(point, bit), w, f);
    return 0;
}

// the unchecked k_ks_mac element (KsMacF64 / KsMacU64 of aux_kernels.hip), for words of any size
int emu_ks_dot_plain(const u64 *x, const u64 *y, int terms, size_t n, u64 q, int path, u64 *w)
{
    if (terms < 1 || (path == PATH_F64 && q >= ((u64)1 << 50))) return -1;
    const LimbParams p = limb(q, path);
    for (size_t i = 0; i < n; i++) {
        if (path == PATH_F64) {
            const ArithF64::Ctx c = ArithF64::make_ctx(p);
            double s = 0.0;
            for (int t = 0; t < terms; t++) {
                const u64 xv = x[(size_t)t * n + i], yv = y[(size_t)t * n + i];
                const double a = ArithF64::from_canonical(xv < q ? xv : xv % q), b = ArithF64::from_canonical(yv < q ? yv : yv % q);
                const double h = a * b;
                const double k = __builtin_rint(a * (b * c.ninv));
                const double l = __builtin_fma(a, b, -h);
                s += __builtin_fma(-k, c.n, h) + l;
                if ((t & 7) == 7) ArithF64::reduce(s, c);
            }
            w[i] = ArithF64::canonical(s, c);
        } else {
            u64 lo = 0, hi = 0;
            for (int t = 0; t < terms; t++) {
                const u64 a = x[(size_t)t * n + i] % q, b = y[(size_t)t * n + i] % q;
                const u64 pl = a * b, ph = mulhi64(a, b);
                lo += pl;
                hi += ph + (lo < pl);
                if ((t & 7) == 7) {
                    lo = barrett128(lo, hi, q, p.barrett_lo, p.barrett_hi);
                    hi = 0;
                }
            }
            w[i] = barrett128(lo, hi, q, p.barrett_lo, p.barrett_hi);
        }
    }
    return 0;
}

// tail element: w[i] = ((x[i] - y[i] mod q) s mod q (+ add[i] when has_add)) mod q
int emu_ks_tail_checked(const u64 *x, const u64 *y, const u64 *add, int has_add, size_t n, u64 q, u64 s, int point, int bit, u64 *w, u32 *f)
{
    if (!ks_tail_point_exists(point < 0 ? 0 : point, has_add != 0)) return -1;
    const LimbParams p = limb(q, PATH_U64);
    const PwFault ft = fault(point, bit);
    const u32 rq = res64(q);
    for (size_t i = 0; i < n; i++)
        w[i] = checked_sub_scale(x[i], true, y[i], true, s, has_add ? add[i] : 0, has_add != 0, q, p.barrett_lo, p.barrett_hi, rq, f[i], ft);
    return 0;
}

// the unchecked k_sub_scale element (aux_kernels.hip), for words of any size
int emu_ks_tail_plain(const u64 *x, const u64 *y, const u64 *add, int has_add, size_t n, u64 q, u64 s, u64 *w)
{
    const LimbParams p = limb(q, PATH_U64);
    const u64 r0 = p.barrett_lo, r1 = p.barrett_hi;
    for (size_t i = 0; i < n; i++) {
        const u64 a = barrett128(x[i], 0, q, r0, r1), b = barrett128(y[i], 0, q, r0, r1);
        const u64 d = a >= b ? a - b : a + q - b;
        u64 v = barrett128(d * s, mulhi64(d, s), q, r0, r1);
        if (has_add) {
            v += barrett128(add[i], 0, q, r0, r1);
            v = v >= q ? v - q : v;
        }
        w[i] = v;
    }
    return 0;
}

} // extern "C"
