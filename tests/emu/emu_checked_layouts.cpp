// emu_checked_layouts.cpp -- the flag layouts of the stage-by-stage checked calls on a host-made plan (TEST INFRASTRUCTURE ONLY).
//
// The layout calls of include/fhe_mi355x.h read a plan's shape and nothing on the device, but a plan can only be created on one.
// This file fills the shape fields of a plan structure on the host (capi_internal.hpp) and calls one of the library's layout
// functions on it, so that their arithmetic can be checked without a GPU.  Host code only; links against libfhe_mi355x.so.
//
//   hipcc -O1 -std=c++17 --cuda-host-only -x hip -shared -fPIC -I<csrc> emu_checked_layouts.cpp -L<pkg> -lfhe_mi355x -o libemu_checked_layouts.so
#include "capi_internal.hpp"

extern "C" {

// which: 0 key switch, 1 BGV key switch, 2 rescale (a = n_parts), 3 BGV mod switch (a = n_parts), 4 multiply (a = rescale), 5 BGV
// multiply (a = rescale), 6 hoisted rotations (a = n_rot), 7 BSGS product (a = n1, b = n2).  out = the call's own array (at most
// 12 words; the caller pre-fills it).  Returns the call's status
int emu_checked_layout(int which, int log_n, int L, int K, int dnum, unsigned long long plain, size_t a, size_t b, int *out)
{
    fhe_keyswitch p;
    p.log_n = log_n;
    p.L = L;
    p.K = K;
    p.dnum = dnum;
    p.alpha = (L + dnum - 1) / dnum;
    p.plain_modulus = plain;
    switch (which) {
    case 0: return fhe_keyswitch_checked_layout(&p, out);
    case 1: return fhe_bgv_keyswitch_checked_layout(&p, out);
    case 2: return fhe_rescale_checked_layout(&p, a, out);
    case 3: return fhe_bgv_mod_switch_checked_layout(&p, a, out);
    case 4: return fhe_hmult_checked_layout(&p, (int)a, out);
    case 5: return fhe_bgv_hmult_checked_layout(&p, (int)a, out);
    case 6: return fhe_rotate_hoisted_checked_layout(&p, a, out);
    case 7: return fhe_bsgs_matvec_checked_layout(&p, a, b, out);
    }
    return -1;
}

} // extern "C"
