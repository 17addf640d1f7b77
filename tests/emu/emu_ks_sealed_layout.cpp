// emu_ks_sealed_layout.cpp -- the flag layout of the sealed key switch on a host-made plan (TEST INFRASTRUCTURE ONLY).
//
// fhe_keyswitch_sealed_layout reads a plan's shape and nothing on the device, but a plan can only be created on one.  As
// emu_checked_layouts.cpp does, this file fills the shape fields of a plan structure on the host (capi_internal.hpp) and calls the
// library's layout function on it.  Host code only; links against libfhe_mi355x.so.
//
//   hipcc -O1 -std=c++17 --cuda-host-only -x hip -shared -fPIC -I<csrc> emu_ks_sealed_layout.cpp -L<pkg> -lfhe_mi355x -o libemu_ks_sealed_layout.so
#include "capi_internal.hpp"

extern "C" {

// out = the call's own array of four words (the caller pre-fills it).  Returns the call's status
int emu_ks_sealed_layout(int log_n, int L, int K, int dnum, unsigned long long plain, int *out)
{
    fhe_keyswitch p;
    p.log_n = log_n;
    p.L = L;
    p.K = K;
    p.dnum = dnum;
    p.alpha = (L + dnum - 1) / dnum;
    p.plain_modulus = plain;
    return fhe_keyswitch_sealed_layout(&p, out);
}

} // extern "C"
