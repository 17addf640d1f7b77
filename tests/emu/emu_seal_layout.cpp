// emu_seal_layout.cpp -- the flag layouts of the sealed composites on a host-made plan (TEST INFRASTRUCTURE ONLY).
//
// The layout calls of include/fhe_mi355x.h read a plan's shape and nothing on the device, but a plan can only be created on one.
// This file fills the shape fields of a plan structure on the host (capi_internal.hpp) and calls the library's layout functions on
// it, so that their arithmetic can be checked without a GPU.  Host code only; links against libfhe_mi355x.so.
//
//   hipcc -O1 -std=c++17 --cuda-host-only -x hip -shared -fPIC -I<csrc> emu_seal_layout.cpp -L<pkg> -lfhe_mi355x -o libemu_seal_layout.so
#include "capi_internal.hpp"

extern "C" {

// sealed[0..7] = fhe_hmult_sealed_layout, sealed[8..13] = fhe_rotate_sealed_layout; inner[0..3] = the checked multiply's layout,
// inner[4] = the checked key switch's total -- the CKKS or the BGV forms, by `plain`.  Returns the first non-zero status
int emu_sealed_layouts(int log_n, int L, int K, int dnum, unsigned long long plain, int rescale, int *sealed, int *inner)
{
    fhe_keyswitch p;
    p.log_n = log_n;
    p.L = L;
    p.K = K;
    p.dnum = dnum;
    p.alpha = (L + dnum - 1) / dnum;
    p.plain_modulus = plain;
    int rc, ks[12];
    if ((rc = fhe_hmult_sealed_layout(&p, rescale, sealed))) return rc;
    if ((rc = fhe_rotate_sealed_layout(&p, sealed + 8))) return rc;
    if (plain) {
        if ((rc = fhe_bgv_hmult_checked_layout(&p, rescale, inner))) return rc;
        if ((rc = fhe_bgv_keyswitch_checked_layout(&p, ks))) return rc;
        inner[4] = ks[10];
    } else {
        if ((rc = fhe_hmult_checked_layout(&p, rescale, inner))) return rc;
        if ((rc = fhe_keyswitch_checked_layout(&p, ks))) return rc;
        inner[4] = ks[8];
    }
    return 0;
}

} // extern "C"
