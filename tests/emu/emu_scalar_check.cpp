// emu_scalar_check.cpp -- CPU emulation of the checked scalar multiply / affine map (TEST INFRASTRUCTURE ONLY).
//
// Compiles fhe_reliability_gpu_amd/csrc/scalar_check.hpp -- the element function the kernel of scalar_checked.hip calls -- with
// g++ and runs it over arrays of words, with an optional bit flip at one injection point of every element, so that words and flag
// bits can be checked against Python integers without a GPU.  The unchecked arithmetic (k_scalar_affine: barrett128 of the 128-bit
// product, plus the addend, one conditional subtraction -- modarith.hpp) is compiled as it is for the words the check cannot
// cover.  The library never links this file.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I<csrc> emu_scalar_check.cpp -o libemu_scalar_check.so
#include "scalar_check.hpp"

using namespace fhe;

namespace {

// floor(2^128 / q) for q not a power of two, as capi.cpp build_tables fills LimbParams::barrett_lo / barrett_hi
void ratio(u64 q, u64 &r0, u64 &r1)
{
    const unsigned __int128 r = ~(unsigned __int128)0 / q;
    r0 = (u64)r;
    r1 = (u64)(r >> 64);
}

} // namespace

extern "C" {

// w[i] = a[i] s (+ o when add) mod q with its flags; point < 0: no fault, else `mask` is XORed into the value at that point of
// every element.  s and o are taken as they are (the library reduces them before the launch)
int emu_scalar_affine_checked(const u64 *a, size_t n, u64 q, u64 s, u64 o, int add, int point, u64 mask, u64 *w, u32 *f)
{
    if (point >= 0 && !scalar_affine_point_exists(point, add != 0)) return -1;
    u64 r0, r1;
    ratio(q, r0, r1);
    const PwFault ft{point, point < 0 ? 0 : mask};
    const u32 rq = res64(q);
    const double ninv = 1.0 / (double)q;      // LimbParams::ninv
    for (size_t i = 0; i < n; i++)
        w[i] = add ? checked_scalar_affine<true>(a[i], s, o, q, r0, r1, ninv, rq, f[i], ft) : checked_scalar_affine<false>(a[i], s, 0, q, r0, r1, ninv, rq, f[i], ft);
    return 0;
}

// the unchecked k_scalar_affine element, for words of any size
int emu_scalar_affine_plain(const u64 *a, size_t n, u64 q, u64 s, u64 o, u64 *w)
{
    u64 r0, r1;
    ratio(q, r0, r1);
    for (size_t i = 0; i < n; i++) {
        const u64 v = barrett128(a[i] * s, mulhi64(a[i], s), q, r0, r1) + o;
        w[i] = v >= q ? v - q : v;
    }
    return 0;
}

} // extern "C"
