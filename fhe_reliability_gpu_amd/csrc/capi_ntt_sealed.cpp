// capi_ntt_sealed.cpp -- the key switch and rotation whose input limbs are verified on the opening transform's own load
// (ntt_seal_tap.hpp, ntt_sealed.hip; the transforms themselves: capi_ntt_fwd_sealed.cpp) -- fhe_keyswitch_apply_sealed_in,
// fhe_rotate_sealed_in, fhe_rotate_sealed_out and their layouts (part of the C ABI of include/fhe_mi355x.h).
//
// fhe_keyswitch_apply_sealed does not seal d_c, and the sealed rotations sweep c0 and c1 and then move them through the unchecked
// permutation: the verifying sweep, the copy into the plan and the opening transform's load are separate loads, and a word that is
// wrong on a later one passes the seal and is a consistent input of the ABFT identity.  Here stage 0 of the checked key switch is the
// sealed inverse transform, out of place from the caller's rows into the plan's coefficient buffer (SealedInputStep,
// capi_checked.hpp): no sweep, no copy.  The rotation is a chain of custody: c0 and c1 are verified on the sealed permutation's
// gather (galois_sealed.hip), sigma(c1)'s seal is written from the registers that are stored, and stage 0 verifies sigma(c1) against
// that seal on the transform's load.  A raised input flag does not stop a call.
#include "capi_sealed.hpp"
#include "galois_seal.hpp"

// one launch per run of an arithmetic path
int KscNtt::launch_sealed(const KscRows &r, const u64 *src, const SealedInputStep &in, int which) const
{
    const fhe_ntt_tables *t = p->t;
    const size_t N = (size_t)1 << p->log_n;
    return for_each_run(t, r.count, r.tl0, [&](size_t off, size_t len, int path) -> int {
        PassArgs pa{r.base + (r.row0 + off) * N, t->d_lp.as<LimbParams>(), (u32)(r.tl0 + off), (u32)len, (u32)len, r.stride, nullptr};
        pa.src = src + (r.row0 + off) * N;
        const size_t slot = (size_t)r.sum0 + r.row0 + off;
        if (r.n_poly != 1 || slot + len > ksc_slots(p)) return fail(FHE_ERR_INVALID, "checked call: a transform's sums lie outside the plan's scratch");
        hipError_t e = launch_ntt_sealed(st, pa, a->win.as<Tw>(), a->wout.as<Tw>(), a->wout8.as<u64>(), sum_in() + slot * tin, sum_out() + slot * tout, p->log_n, path,
                                         which, true, run_seal_in(in, off, len, r.count, tin), nullptr);
        return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_ntt_sealed");
    });
}

extern "C" {

int fhe_keyswitch_sealed_in_layout(const fhe_keyswitch *p, int out[5]) { return ks_sealed_layout(p, 1, true, out); }

int fhe_keyswitch_apply_sealed_in(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c, const uint64_t *d_evk,
                                  const uint64_t *d_add0, const uint64_t *d_add1, const fhe_abft *a, const uint64_t *d_seal_c, const uint64_t *d_seal_key,
                                  uint32_t *d_flags, void *stream)
{
    const KsSealedCall c{ctx, p, d_out0, d_out1, d_c, d_evk, d_add0, d_add1, a, d_seal_key, d_flags, stream, 1, d_seal_c, nullptr};
    KsSealed k;
    const int rc = ks_sealed_open(c, k);
    return rc ? rc : ks_sealed_run(c, k, d_c, d_add0);
}

int fhe_rotate_sealed_in_layout(const fhe_keyswitch *p, int out[7]) { return ks_sealed_layout(p, 3, true, out); }

} // extern "C"

// fhe_rotate_sealed_in, and fhe_rotate_sealed_out (out): the two output sweeps are gone and the key switch's stage 7 is the sealed
// tail (capi_subscale_sealed.cpp), which writes the outputs' seals from the registers it stores; the call takes that step's hook
static int rotate_sealed_in_body(bool out, fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1,
                                 uint32_t galois_elt, const uint64_t *d_galois_key, const fhe_abft *a, const uint64_t *const *d_seal_in, const uint64_t *d_seal_key,
                                 uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream)
{
    const KsSealedRotation rot{galois_elt, d_seal_in, d_seal_out, out};
    const KsSealedCall c{ctx, p, d_out0, d_out1, d_c1, d_galois_key, d_c0, nullptr, a, d_seal_key, d_flags, stream, 3, nullptr, &rot};
    KsSealed k;
    int rc = ks_sealed_open(c, k);
    if (rc) return rc;
    const size_t L = (size_t)p->L, N = (size_t)1 << p->log_n;
    // sigma(c0) and sigma(c1) into the plan's buffers through the sealed permutation: both verified on the gather, sigma(c1)'s seal
    // written from the registers that are stored (it lives behind the partials until stage 0 ends)
    u64 *sig1 = p->rot.as<u64>(), *sig0 = sig1 + L * N, *seal_sig1 = k.behind;
    const LimbParams *lp = p->t->d_lp.as<LimbParams>();
    const GalSealHit no_hit{-1, 0, 0, 0};
    const GalSealArgs g0{sig0, d_c0, lp, 0u, (u32)L, (u32)L, (u32)L, p->log_n, galois_elt}, g1{sig1, d_c1, lp, 0u, (u32)L, (u32)L, (u32)L, p->log_n, galois_elt};
    hipError_t e = launch_automorphism_ntt_sealed(k.st, g0, k.part, d_seal_in[0], nullptr, d_flags + k.lay[0], no_hit);
    if (e == hipSuccess) e = launch_automorphism_ntt_sealed(k.st, g1, k.part, d_seal_in[1], seal_sig1, d_flags + k.lay[1], no_hit);
    if (e != hipSuccess) return hip_fail(e, "launch_automorphism_ntt_sealed");
    k.in.seal = seal_sig1;
    if ((rc = ks_sealed_run(c, k, sig1, sig0)) || out) return rc;
    return seal_outputs(k.st, p->t, d_seal_out, nullptr, d_out0, d_out1, L, k.part);
}

extern "C" {

int fhe_rotate_sealed_in(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1, uint32_t galois_elt,
                         const uint64_t *d_galois_key, const fhe_abft *a, const uint64_t *const *d_seal_in, const uint64_t *d_seal_key,
                         uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream)
{
    return rotate_sealed_in_body(false, ctx, p, d_out0, d_out1, d_c0, d_c1, galois_elt, d_galois_key, a, d_seal_in, d_seal_key, d_seal_out, d_flags, stream);
}

int fhe_rotate_sealed_out(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1, uint32_t galois_elt,
                          const uint64_t *d_galois_key, const fhe_abft *a, const uint64_t *const *d_seal_in, const uint64_t *d_seal_key,
                          uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream)
{
    return rotate_sealed_in_body(true, ctx, p, d_out0, d_out1, d_c0, d_c1, galois_elt, d_galois_key, a, d_seal_in, d_seal_key, d_seal_out, d_flags, stream);
}

} // extern "C"
