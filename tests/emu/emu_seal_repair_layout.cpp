// emu_seal_repair_layout.cpp -- the flag layouts of the repairing composites on a host-made plan (TEST INFRASTRUCTURE ONLY).
//
// As emu_seal_layout.cpp: the layout calls of include/fhe_mi355x.h read a plan's shape and nothing on the device, so this file
// fills the shape fields of a plan structure on the host (capi_internal.hpp) and calls the library's layout functions on it.
// Host code only; links against libfhe_mi355x.so.
//
//   hipcc -O1 -std=c++17 --cuda-host-only -x hip -shared -fPIC -I<csrc> emu_seal_repair_layout.cpp -L<pkg> -lfhe_mi355x -o libemu_seal_repair_layout.so
#include "capi_internal.hpp"

extern "C" {

// sealed[0..7] = fhe_hmult_sealed_layout, sealed[8..13] = fhe_rotate_sealed_layout; repair[0..9] = fhe_hmult_sealed_repair_layout,
// repair[10..17] = fhe_rotate_sealed_repair_layout.  Returns the first non-zero status
int emu_repair_layouts(int log_n, int L, int K, int dnum, unsigned long long plain, int rescale, int *sealed, int *repair)
{
    fhe_keyswitch p;
    p.log_n = log_n;
    p.L = L;
    p.K = K;
    p.dnum = dnum;
    p.alpha = (L + dnum - 1) / dnum;
    p.plain_modulus = plain;
    int rc;
    if ((rc = fhe_hmult_sealed_layout(&p, rescale, sealed))) return rc;
    if ((rc = fhe_rotate_sealed_layout(&p, sealed + 8))) return rc;
    if ((rc = fhe_hmult_sealed_repair_layout(&p, rescale, repair))) return rc;
    if ((rc = fhe_rotate_sealed_repair_layout(&p, repair + 10))) return rc;
    return 0;
}

} // extern "C"
