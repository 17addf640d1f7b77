// emu_rescale_sealed_layout.cpp -- the flag layout of the sealed rescale on a host-made plan, and the refusal of a null input seal on
// a host-made context (TEST INFRASTRUCTURE ONLY).
//
// The layout call reads a plan's shape and nothing on the device, and the null-seal refusal happens before any device work, but a
// plan and a context can only be created on a device.  As emu_ntt_sealed_layout.cpp does, this file fills the shape fields of the
// structures on the host (capi_internal.hpp) and calls the library on them.  Host code only; links against libfhe_mi355x.so.
//
//   hipcc -O1 -std=c++17 --cuda-host-only -x hip -shared -fPIC -I<csrc> emu_rescale_sealed_layout.cpp -L<pkg> -lfhe_mi355x -o libemu_rescale_sealed_layout.so
#include "capi_internal.hpp"

namespace {

void shape(fhe_keyswitch &p, int log_n, int L, int K, int dnum, unsigned long long plain)
{
    p.log_n = log_n;
    p.L = L;
    p.K = K;
    p.dnum = dnum;
    p.alpha = (L + dnum - 1) / dnum;
    p.plain_modulus = plain;
}

} // namespace

extern "C" {

// fhe_rescale_sealed_layout (four words) and, behind it, the checked rescale's layout of the same form (up to eight words); out is
// pre-filled by the caller
int emu_rescale_sealed_layout(int log_n, int L, int K, int dnum, unsigned long long plain, int n_parts, int *out, int *inner)
{
    fhe_keyswitch p;
    shape(p, log_n, L, K, dnum, plain);
    const int rc = plain ? fhe_bgv_mod_switch_checked_layout(&p, (size_t)n_parts, inner) : fhe_rescale_checked_layout(&p, (size_t)n_parts, inner);
    if (rc) return rc;
    return fhe_rescale_sealed_layout(&p, (size_t)n_parts, out);
}

// arms the sealed tail's hook on a host-made context, calls fhe_rescale_sealed with every pointer set but d_seal_in, and reports {the
// call's status, the hook's point before the call, the hook's point after it, the flag word untouched}
int emu_null_seal_in(int log_n, int L, int K, int dnum, int *out)
{
    fhe_ctx ctx;
    fhe_keyswitch p;
    shape(p, log_n, L, K, dnum, 0);
    p.ctx = &ctx;
    alignas(16) static uint64_t dummy[4];
    uint32_t flags[1] = {0x5A5A5A5Au};
    int rc = fhe_ctx_inject_fault_subscale_sealed(&ctx, 1, 2, 3, 4);
    if (rc) return rc;
    out[1] = ctx.subscale_seal_fault.sel;
    out[0] = fhe_rescale_sealed(&ctx, &p, dummy, dummy + 2, 2, reinterpret_cast<const fhe_abft *>(dummy), nullptr, dummy, flags, nullptr);
    out[2] = ctx.subscale_seal_fault.sel;
    out[3] = flags[0] == 0x5A5A5A5Au;
    return 0;
}

} // extern "C"
