// emu_rescale_check.cpp -- CPU emulation of the checked rescale's residue stage (TEST INFRASTRUCTURE ONLY).
//
// Compiles fhe_reliability_gpu_amd/csrc/rescale_check.hpp -- the element function the kernel of rescale_checked.hip calls --
// with g++ and runs it over arrays of words, with an optional bit flip at one injection point of every element, so that words
// and flag bits can be checked against Python integers without a GPU.  The unchecked arithmetic (barrett128(x, 0, q) of
// modarith.hpp) is called as it is for the words the check cannot cover.  The library never links this file.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I<csrc> emu_rescale_check.cpp -o libemu_rescale_check.so
#include "rescale_check.hpp"

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

// w[i] = x[i] mod q with its flags; point < 0: no fault, else `mask` is XORed into the value at that point of every element
int emu_rescale_reduce_checked(const u64 *x, size_t n, u64 qlast, u64 q, int point, u64 mask, u64 *w, u32 *f)
{
    if (point >= 0 && !rescale_reduce_point_exists(point)) return -1;
    u64 r0, r1;
    ratio(q, r0, r1);
    const PwFault ft{point, point < 0 ? 0 : mask};
    const u32 rq = res64(q);
    for (size_t i = 0; i < n; i++) w[i] = checked_reduce_word(x[i], qlast, q, r0, r1, res64(x[i]), rq, f[i], ft);
    return 0;
}

// the unchecked arithmetic, for words of any size
int emu_rescale_reduce_plain(const u64 *x, size_t n, u64 q, u64 *w)
{
    u64 r0, r1;
    ratio(q, r0, r1);
    for (size_t i = 0; i < n; i++) w[i] = barrett128(x[i], 0, q, r0, r1);
    return 0;
}

} // extern "C"
