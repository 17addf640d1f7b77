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

int fhe_keyswitch_sealed_in_layout(const fhe_keyswitch *p, int out[5])
{
    if (!p || !out) return fail(FHE_ERR_INVALID, "null argument");
    out[0] = 0;
    out[1] = p->L;
    out[2] = out[1] + (int)key_rows(p);
    out[3] = out[2] + ksc_layout(p, sealed_form(p).form).total;
    out[4] = ks_sealed_fused(p) ? 1 : 0;
    return FHE_OK;
}

int fhe_keyswitch_apply_sealed_in(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c, const uint64_t *d_evk,
                                  const uint64_t *d_add0, const uint64_t *d_add1, const fhe_abft *a, const uint64_t *d_seal_c, const uint64_t *d_seal_key,
                                  uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    const SealedForm f = sealed_form(p);
    const KsForm form = f.form;
    // the three hooks belong to this call whatever its outcome
    const StagedFault ft = (ctx->*f.ks_hook).take();
    const SealHook kf = ctx->ks_seal_fault.take();
    const SealHook nf = ctx->ntt_seal_fault.take();
    if (!d_seal_c) return fail(FHE_ERR_INVALID, "null d_seal_c: nothing would verify the input limbs (fhe_keyswitch_apply_sealed takes none)");
    int rc = ksc_scope(ctx, p, a, d_flags, form, false);
    if (rc) return rc;
    if (!d_out0 || !d_out1 || !d_c || !d_evk) return fail(FHE_ERR_INVALID, "null argument");
    if (d_out0 == d_out1) return fail(FHE_ERR_INVALID, "the two output parts must be distinct buffers");
    if (misaligned({d_out0, d_out1, d_c, d_evk, d_add0, d_add1}))
        return fail(FHE_ERR_INVALID, "sealed rows are read 16 bytes at a time: the buffers must be 16-byte aligned");
    int lay[5];
    if ((rc = fhe_keyswitch_sealed_in_layout(p, lay))) return rc;
    SealedKeyStep key{d_seal_key, d_flags + lay[1], nullptr, KsSealHit{0, 0, 0}};
    SealedInputStep in{d_seal_c, d_flags + lay[0], nullptr, 0, 0, 0};
    if ((rc = ks_seal_hit(kf, p, key.hit))) return rc;
    if ((rc = ntt_seal_hit(nf, (size_t)p->L, p->log_n, in))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    // the checked key switch's own hook, against the call: before anything is launched (keyswitch_checked checks it again)
    if ((rc = ksc_prepare(p))) return rc;
    KscHook h;
    if ((rc = ksc_hook(p, form, ft, p->acc.as<u64>(), d_add0 != nullptr, d_add1 != nullptr, h))) return rc;
    hipStream_t st = pick(ctx, stream);
    u64 *part;
    if ((rc = seal_scratch(ctx, st, std::max(ks_sealed_scratch_words(p), ntt_seal_part_words((u32)p->L, p->log_n, true)), &part))) return rc;
    key.part = in.part = part;      // stage 0's verdict is out before stage 3 starts on the same stream
    HIP_TRY(hipMemsetAsync(d_flags, 0, (size_t)lay[2] * sizeof(u32), st));
    return keyswitch_checked(p, form, d_out0, d_out1, d_c, d_evk, d_add0, d_add1, a, d_flags + lay[2], st, ft, &key, &in);
}

int fhe_rotate_sealed_in_layout(const fhe_keyswitch *p, int out[7])
{
    if (!p || !out) return fail(FHE_ERR_INVALID, "null argument");
    out[0] = 0;
    out[1] = p->L;
    out[2] = 2 * p->L;
    out[3] = 3 * p->L;
    out[4] = out[3] + (int)key_rows(p);
    out[5] = out[4] + ksc_layout(p, sealed_form(p).form).total;
    out[6] = ks_sealed_fused(p) ? 1 : 0;
    return FHE_OK;
}

} // extern "C"

// fhe_rotate_sealed_in, and fhe_rotate_sealed_out (out): the two output sweeps are gone and the key switch's stage 7 is the sealed
// tail (capi_subscale_sealed.cpp), which writes the outputs' seals from the registers it stores; the call takes that step's hook
static int rotate_sealed_in_body(bool out, fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1,
                                 uint32_t galois_elt, const uint64_t *d_galois_key, const fhe_abft *a, const uint64_t *const *d_seal_in, const uint64_t *d_seal_key,
                                 uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    const SealedForm f = sealed_form(p);
    const KsForm form = f.form;
    const StagedFault ft = (ctx->*f.ks_hook).take();
    const SealHook kf = ctx->ks_seal_fault.take();
    const SealHook nf = ctx->ntt_seal_fault.take();
    const SealHook tf = out ? ctx->subscale_seal_fault.take() : SealHook{};
    int rc = ksc_scope(ctx, p, a, d_flags, form, false);
    if (rc) return rc;
    if (!d_out0 || !d_out1 || !d_c0 || !d_c1 || !d_galois_key) return fail(FHE_ERR_INVALID, "null argument");
    if (!d_seal_in || !d_seal_in[0] || !d_seal_in[1]) return fail(FHE_ERR_INVALID, "null seal of c0 or c1: nothing would verify the permutation's source");
    if (d_out0 == d_out1) return fail(FHE_ERR_INVALID, "the two output parts must be distinct buffers");
    if (!(galois_elt & 1)) return fail(FHE_ERR_INVALID, "Galois elements are odd");
    if (p->log_n < 1) return fail(FHE_ERR_UNSUPPORTED, "a sealed row has at least two words");
    if (misaligned({d_out0, d_out1, d_c0, d_c1, d_galois_key}))
        return fail(FHE_ERR_INVALID, "sealed rows are read 16 bytes at a time: the buffers must be 16-byte aligned");
    int lay[7];
    if ((rc = fhe_rotate_sealed_in_layout(p, lay))) return rc;
    SealedKeyStep key{d_seal_key, d_flags + lay[3], nullptr, KsSealHit{0, 0, 0}};
    SealedInputStep in{nullptr, d_flags + lay[2], nullptr, 0, 0, 0};
    if ((rc = ks_seal_hit(kf, p, key.hit))) return rc;
    if ((rc = ntt_seal_hit(nf, (size_t)p->L, p->log_n, in))) return rc;
    SealedTailStep tail{{d_seal_out ? d_seal_out[0] : nullptr, d_seal_out ? d_seal_out[1] : nullptr, nullptr}, nullptr};
    if (out && (rc = subscale_seal_hit(tf, 2, 0, tail.seal_out[0] && tail.seal_out[1] ? (size_t)p->L : 0, p->log_n, tail))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = ksc_prepare(p))) return rc;
    KscHook h;
    if ((rc = ksc_hook(p, form, ft, p->acc.as<u64>(), true, false, h))) return rc;
    hipStream_t st = pick(ctx, stream);
    const size_t L = (size_t)p->L, N = (size_t)1 << p->log_n;
    // the launches' partials share one region (stream order keeps them apart); sigma(c1)'s seal lives behind it until stage 0 ends
    const size_t pw = std::max(std::max(ks_sealed_scratch_words(p), ntt_seal_part_words((u32)L, p->log_n, true)),
                               std::max(galois_seal_part_words((u32)L, p->log_n, true), seal_part_words((u32)L, p->log_n)));
    u64 *part;
    if ((rc = seal_scratch(ctx, st, pw + 2 * L, &part))) return rc;
    u64 *seal_sig1 = part + pw;
    key.part = in.part = tail.part = part;      // the tail's partials, [2 L][chunks][2], are fewer than the key's
    in.seal = seal_sig1;
    HIP_TRY(hipMemsetAsync(d_flags, 0, (size_t)lay[4] * sizeof(u32), st));
    // sigma(c0) and sigma(c1) into the plan's buffers through the sealed permutation: both verified on the gather, sigma(c1)'s seal
    // written from the registers that are stored
    u64 *sig1 = p->rot.as<u64>(), *sig0 = sig1 + L * N;
    const LimbParams *lp = p->t->d_lp.as<LimbParams>();
    const GalSealHit no_hit{-1, 0, 0, 0};
    const GalSealArgs g0{sig0, d_c0, lp, 0u, (u32)L, (u32)L, (u32)L, p->log_n, galois_elt}, g1{sig1, d_c1, lp, 0u, (u32)L, (u32)L, (u32)L, p->log_n, galois_elt};
    hipError_t e = launch_automorphism_ntt_sealed(st, g0, part, d_seal_in[0], nullptr, d_flags + lay[0], no_hit);
    if (e == hipSuccess) e = launch_automorphism_ntt_sealed(st, g1, part, d_seal_in[1], seal_sig1, d_flags + lay[1], no_hit);
    if (e != hipSuccess) return hip_fail(e, "launch_automorphism_ntt_sealed");
    if ((rc = keyswitch_checked(p, form, d_out0, d_out1, sig1, d_galois_key, sig0, nullptr, a, d_flags + lay[4], st, ft, &key, &in, out ? &tail : nullptr)) || out)
        return rc;
    return seal_outputs(st, p->t, d_seal_out, nullptr, d_out0, d_out1, L, part);
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
