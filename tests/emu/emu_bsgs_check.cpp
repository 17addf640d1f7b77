// emu_bsgs_check.cpp -- CPU emulation of the checked inner sum of the BSGS product and of the checked add (TEST INFRASTRUCTURE ONLY).
//
// Compiles fhe_reliability_gpu_amd/csrc/bsgs_check.hpp -- the element functions the kernels of bsgs_checked.hip call -- with g++ and
// runs them over arrays of elements, with an optional bit flip at one injection point of one ciphertext part of every element, so
// that words and flag bits can be checked against Python integers without a GPU.  The unchecked elements (k_diag_mac with KsMacU64 /
// KsMacF64, k_modadd of aux_kernels.hip) are restated here for the operands the checks cannot cover.  The library never links this
// file.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I<csrc> emu_bsgs_check.cpp -o libemu_bsgs_check.so
#include "bsgs_check.hpp"

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
void diag_checked(const u64 *d, const u64 *y0, const u64 *y1, int n1, size_t n, const LimbParams &p, const PwFault &f0, const PwFault &f1, u64 *w0, u64 *w1,
                  u32 *fl0, u32 *fl1)
{
    for (size_t i = 0; i < n; i++) {
        DiagDot<D> s;
        for (int b = 0; b < n1; b++) s.mac(d[(size_t)b * n + i], y0[(size_t)b * n + i], y1[(size_t)b * n + i], (u32)b, p, f0, f1);
        s.finish((u32)n1, p, w0[i], w1[i], fl0[i], fl1[i], f0, f1);
    }
}

// one part of the unchecked k_diag_mac element: K::mac(s, d, y, b, p) over the baby steps, K::out
u64 diag_plain(const u64 *d, const u64 *y, int n1, size_t n, size_t i, const LimbParams &p)
{
    const u64 q = p.q;
    if (p.path == PATH_F64) {
        const ArithF64::Ctx c = ArithF64::make_ctx(p);
        double s = 0.0;
        for (int t = 0; t < n1; t++) {
            const u64 xv = d[(size_t)t * n + i], yv = y[(size_t)t * n + i];
            const double a = ArithF64::from_canonical(xv < q ? xv : xv % q), b = ArithF64::from_canonical(yv < q ? yv : yv % q);
            const double h = a * b;
            const double k = __builtin_rint(a * (b * c.ninv));
            const double l = __builtin_fma(a, b, -h);
            s += __builtin_fma(-k, c.n, h) + l;
            if ((t & 7) == 7) ArithF64::reduce(s, c);
        }
        return ArithF64::canonical(s, c);
    }
    u64 lo = 0, hi = 0;
    for (int t = 0; t < n1; t++) {
        const u64 a = d[(size_t)t * n + i] % q, b = y[(size_t)t * n + i] % q;
        const u64 pl = a * b, ph = mulhi64(a, b);
        lo += pl;
        hi += ph + (lo < pl);
        if ((t & 7) == 7) {
            lo = barrett128(lo, hi, q, p.barrett_lo, p.barrett_hi);
            hi = 0;
        }
    }
    return barrett128(lo, hi, q, p.barrett_lo, p.barrett_hi);
}

} // namespace

extern "C" {

// inner sum over n1 baby steps per element and part: d = [n1][n] diagonal words, y0 / y1 = [n1][n] words of the two parts; path 0 =
// FP64-term form (q < 2^50), 1 = U64.  The flip (point >= 0) hits part `half` only
int emu_diag_mac_checked(const u64 *d, const u64 *y0, const u64 *y1, int n1, size_t n, u64 q, int path, int half, int point, int bit, u64 *w0, u64 *w1,
                         u32 *fl0, u32 *fl1)
{
    if (n1 < 1 || (path == PATH_F64 && q >= ((u64)1 << 50)) || point > 3 || (half != 0 && half != 1)) return -1;
    const LimbParams p = limb(q, path);
    const PwFault none = fault(-1, 0), f = fault(point, bit);
    const PwFault &f0 = half == 0 ? f : none, &f1 = half == 1 ? f : none;
    if (path == PATH_F64) diag_checked<KsDotF64>(d, y0, y1, n1, n, p, f0, f1, w0, w1, fl0, fl1);
    else diag_checked<KsDotU64>(d, y0, y1, n1, n, p, f0, f1, w0, w1, fl0, fl1);
    return 0;
}

// the unchecked k_diag_mac element, for words of any size
int emu_diag_mac_plain(const u64 *d, const u64 *y0, const u64 *y1, int n1, size_t n, u64 q, int path, u64 *w0, u64 *w1)
{
    if (n1 < 1 || (path == PATH_F64 && q >= ((u64)1 << 50))) return -1;
    const LimbParams p = limb(q, path);
    for (size_t i = 0; i < n; i++) {
        w0[i] = diag_plain(d, y0, n1, n, i, p);
        w1[i] = diag_plain(d, y1, n1, n, i, p);
    }
    return 0;
}

// add element: w[i] = (a[i] + b[i]) mod q; points 2 (the word) and 3 (a + b) exist, 0 and 1 are refused
int emu_modadd_checked(const u64 *a, const u64 *b, size_t n, u64 q, int point, int bit, u64 *w, u32 *f)
{
    if (point >= 0 && !modadd_point_exists(point)) return -1;
    const LimbParams p = limb(q, PATH_U64);
    const PwFault ft = fault(point, bit);
    const u32 rq = res64(q);
    for (size_t i = 0; i < n; i++) w[i] = checked_modadd(a[i], b[i], q, p.barrett_lo, p.barrett_hi, rq, f[i], ft);
    return 0;
}

// the unchecked k_modadd element (aux_kernels.hip), for words of any size
int emu_modadd_plain(const u64 *a, const u64 *b, size_t n, u64 q, u64 *w)
{
    const LimbParams p = limb(q, PATH_U64);
    for (size_t i = 0; i < n; i++) {
        const u64 s = barrett128(a[i], 0, q, p.barrett_lo, p.barrett_hi) + barrett128(b[i], 0, q, p.barrett_lo, p.barrett_hi);
        w[i] = s >= q ? s - q : s;
    }
    return 0;
}

} // extern "C"
