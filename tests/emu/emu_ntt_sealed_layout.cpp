// emu_ntt_sealed_layout.cpp -- the flag layouts of the input-sealed key switch and rotation on a host-made plan, and the refusal of
// a null input seal on a host-made context (TEST INFRASTRUCTURE ONLY).
//
// The layout calls read a plan's shape and nothing on the device, and the null-seal refusal happens before any device work, but a
// plan and a context can only be created on a device.  As emu_ks_sealed_layout.cpp does, this file fills the shape fields of the
// structures on the host (capi_internal.hpp) and calls the library on them.  Host code only; links against libfhe_mi355x.so.
//
//   hipcc -O1 -std=c++17 --cuda-host-only -x hip -shared -fPIC -I<csrc> emu_ntt_sealed_layout.cpp -L<pkg> -lfhe_mi355x -o libemu_ntt_sealed_layout.so
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

// which = 0: fhe_keyswitch_sealed_in_layout (five words), 1: fhe_rotate_sealed_in_layout (seven words); out is pre-filled by the caller
int emu_ntt_sealed_layout(int which, int log_n, int L, int K, int dnum, unsigned long long plain, int *out)
{
    fhe_keyswitch p;
    shape(p, log_n, L, K, dnum, plain);
    return which ? fhe_rotate_sealed_in_layout(&p, out) : fhe_keyswitch_sealed_in_layout(&p, out);
}

// arms the sealed transform's hook on a host-made context, calls fhe_keyswitch_apply_sealed_in with every pointer set but d_seal_c,
// and reports {the call's status, the hook's row before the call, the hook's row after it}
int emu_null_seal_c(int log_n, int L, int K, int dnum, int *out)
{
    fhe_ctx ctx;
    fhe_keyswitch p;
    shape(p, log_n, L, K, dnum, 0);
    p.ctx = &ctx;
    alignas(16) static uint64_t dummy[4];
    uint32_t flags[1] = {0x5A5A5A5Au};
    int rc = fhe_ctx_inject_fault_ntt_sealed(&ctx, 1, 2, 3);
    if (rc) return rc;
    out[1] = ctx.ntt_seal_fault.sel;
    out[0] = fhe_keyswitch_apply_sealed_in(&ctx, &p, dummy, dummy + 2, dummy, dummy, nullptr, nullptr, reinterpret_cast<const fhe_abft *>(dummy), nullptr, dummy, flags,
                                           nullptr);
    out[2] = ctx.ntt_seal_fault.sel;
    out[3] = flags[0] == 0x5A5A5A5Au;
    return 0;
}

} // extern "C"
