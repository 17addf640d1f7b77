// emu_pointwise.cpp -- CPU emulation of the residue-checked element-wise products (TEST INFRASTRUCTURE ONLY).
//
// Compiles fhe_reliability_gpu_amd/csrc/residue_check.hpp -- the element functions the kernels of pointwise_checked.hip
// call -- with g++ and runs them over arrays of elements, with an optional bit flip at one injection point of every
// element, so that words and flag bits can be checked against Python integers without a GPU.  The library never links
// this file.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I<csrc> emu_pointwise.cpp -o libemu_pointwise.so
#include "residue_check.hpp"

using namespace fhe;

namespace {

// the limb constants as capi.cpp build_tables fills them (the fields these products read)
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

} // namespace

extern "C" {

// Barrett form (k_modmul_checked): w[i] = a[i] b[i] (+ o[i] when acc) mod q, f[i] = flag bits; point < 0: no fault
int emu_modmul_checked(const u64 *a, const u64 *b, const u64 *o, size_t n, u64 q, int acc, int point, int bit, u64 *w, u32 *f)
{
    const LimbParams p = limb(q, PATH_U64);
    const PwFault ft = fault(point, bit);
    const u32 rq = res64(q);
    for (size_t i = 0; i < n; i++)
        w[i] = acc ? checked_modmul_barrett<true>(a[i], b[i], o[i], q, p.barrett_lo, p.barrett_hi, rq, f[i], ft)
                   : checked_modmul_barrett<false>(a[i], b[i], 0, q, p.barrett_lo, p.barrett_hi, rq, f[i], ft);
    return 0;
}

// the unchecked k_modmul element (aux_kernels.hip mulmod_b + accumulate), for words of any size
int emu_modmul_plain(const u64 *a, const u64 *b, const u64 *o, size_t n, u64 q, int acc, u64 *w)
{
    const LimbParams p = limb(q, PATH_U64);
    for (size_t i = 0; i < n; i++) {
        u64 c = barrett128(a[i] * b[i], mulhi64(a[i], b[i]), q, p.barrett_lo, p.barrett_hi);
        if (acc) {
            const u64 x = c + barrett128(o[i], 0, q, p.barrett_lo, p.barrett_hi);
            c = x >= q ? x - q : x;
        }
        w[i] = c;
    }
    return 0;
}

// sum of `terms` (1 or 2) products per element, x = [terms][n], y = [terms][n]; path 0 = FP64-term form (q < 2^50), 1 = U64
int emu_dot_checked(const u64 *x, const u64 *y, int terms, size_t n, u64 q, int path, int point, int bit, u64 *w, u32 *f)
{
    if (terms < 1 || terms > 2 || (path == PATH_F64 && q >= ((u64)1 << 50))) return -1;
    const LimbParams p = limb(q, path);
    const PwFault ft = fault(point, bit);
    for (size_t i = 0; i < n; i++) {
        if (terms == 1) {
            const u64 xs[1] = {x[i]}, ys[1] = {y[i]};
            w[i] = path == PATH_F64 ? checked_dot_f64<1>(xs, ys, p, f[i], ft) : checked_dot_u64<1>(xs, ys, p, f[i], ft);
        } else {
            const u64 xs[2] = {x[i], x[n + i]}, ys[2] = {y[i], y[n + i]};
            w[i] = path == PATH_F64 ? checked_dot_f64<2>(xs, ys, p, f[i], ft) : checked_dot_u64<2>(xs, ys, p, f[i], ft);
        }
    }
    return 0;
}

} // extern "C"
