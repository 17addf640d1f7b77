// emu_hoisted_sealed_layout.cpp -- the flag layout of the sealed hoisted rotations on a host-made plan (TEST INFRASTRUCTURE ONLY).
//
// fhe_rotate_hoisted_sealed_layout reads a plan's shape and nothing on the device, but a plan can only be created on one.  As
// emu_ks_sealed_layout.cpp does, this file fills the shape fields of a plan structure on the host (capi_internal.hpp) and calls the
// library's layout functions on it; the refusal of a null source seal is shown on a host-made context in the same way.  Host code
// only; links against libfhe_mi355x.so.
//
//   hipcc -O1 -std=c++17 --cuda-host-only -x hip -shared -fPIC -I<csrc> emu_hoisted_sealed_layout.cpp -L<pkg> -lfhe_mi355x -o libemu_hoisted_sealed_layout.so
#include "capi_internal.hpp"

extern "C" {

// out = the sealed call's own array of six words, checked = fhe_rotate_hoisted_checked_layout's twelve (the caller pre-fills both).
// Returns the sealed layout call's status; *rc_checked = the checked layout call's
int emu_hoisted_sealed_layout(int log_n, int L, int K, int dnum, unsigned long long plain, unsigned long long n_rot, int *out, int *checked, int *rc_checked)
{
    fhe_keyswitch p;
    p.log_n = log_n;
    p.L = L;
    p.K = K;
    p.dnum = dnum;
    p.alpha = (L + dnum - 1) / dnum;
    p.plain_modulus = plain;
    *rc_checked = fhe_rotate_hoisted_checked_layout(&p, (size_t)n_rot, checked);
    return fhe_rotate_hoisted_sealed_layout(&p, (size_t)n_rot, out);
}

// fhe_automorphism_ntt_sealed on a host-made context (never destroyed: it owns nothing) with every buffer given except the
// source's seal: the call must refuse before it looks at tables or device.  An armed hook goes with the refused call: *armed_after =
// is the hook still armed afterwards.  Returns the call's status
int emu_sealed_null_source_seal(int *armed_after)
{
    static fhe_ctx *ctx = new fhe_ctx;
    alignas(16) static uint64_t words[8];
    static uint32_t flags[2];
    fhe_ctx_inject_fault_galois_sealed(ctx, 0, 0, 0, 0, 0);
    const int rc = fhe_automorphism_ntt_sealed(ctx, words, words + 4, words + 2, nullptr, nullptr, 1, 1, 0, 3, flags, nullptr);
    *armed_after = ctx->gal_seal_fault.sel >= 0 ? 1 : 0;
    return rc;
}

} // extern "C"
