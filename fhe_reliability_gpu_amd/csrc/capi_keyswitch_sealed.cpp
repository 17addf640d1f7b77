// capi_keyswitch_sealed.cpp -- the key switch with the switching key verified on the load that multiplies it (ks_seal.hpp,
// keyswitch_sealed.hip): fhe_keyswitch_apply_sealed, its layout and its test hook (part of the C ABI of include/fhe_mi355x.h), and
// the sealed stage 3 behind them as a step of a composite (fhe_rotate_sealed_fused, fhe_hmult_sealed_fused_key, capi_seal.cpp).
//
// The sealed composites verify the key's rows in a sweep of their own and the checked key switch multiplies from a second load.
// Here the inner product loads every key word once, digests it from the register that is handed to the product, and a finish
// launch holds the rows' sums against the stored seal.  The flag buffer of fhe_keyswitch_apply_sealed is
//     [key rows, [dnum][2][M]][the checked key switch's own block, exactly its layout]
// and a raised key flag does not stop the call: the words are the product of the key as it was loaded, and the residue identity
// holds on them.  The ciphertext d_c is not sealed here: its consuming loads are inside the transform kernels of stage 0.
//
// Above KS_SEAL_MAX_DNUM digits there is no fused instantiation: the stage is then the verifying sweep over the key's rows followed
// by the checked inner product, writing the same flag words (a key without a stored seal is then not swept at all, as in the
// sweep-based composites; on the fused route its window is checked all the same).
#include "capi_sealed.hpp"
#include "ks_seal.hpp"

bool ks_sealed_fused(const fhe_keyswitch *p) { return p->dnum >= 1 && (u32)p->dnum <= KS_SEAL_MAX_DNUM && p->log_n >= 1; }

// either route: the partials of the fused launch are [M][chunks][2 dnum][2], those of the sweep [dnum 2 M][chunks][2]
size_t ks_sealed_scratch_words(const fhe_keyswitch *p)
{
    return std::max(ks_seal_part_words((u32)(p->L + p->K), p->log_n, (u32)p->dnum), seal_part_words((u32)key_rows(p), p->log_n));
}

int ks_seal_hit(const SealHook &f, const fhe_keyswitch *p, KsSealHit &hit)
{
    hit = KsSealHit{0, 0, 0};
    if (f.sel < 0) return FHE_OK;
    if (!f.inside(key_rows(p), p->log_n)) return fail(FHE_ERR_INVALID, "fault key row or word outside the call");
    if (!ks_sealed_fused(p)) return fail(FHE_ERR_INVALID, "fault outside the call: above the fused cap no load of the inner product digests the key");
    hit = KsSealHit{(u32)f.row, (u64)f.coeff, (u64)1 << f.bit};
    return FHE_OK;
}

int ks_mac_sealed_stage(const fhe_keyswitch *p, hipStream_t st, const KsMacArgs &ka, const BcCheck &k, const SealedKeyStep &key)
{
    hipError_t e;
    if (ks_sealed_fused(p)) {
        e = launch_ks_mac_sealed(st, ka, key.part, key.seal_key, key.flags_key, k, key.hit);
        return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_ks_mac_sealed");
    }
    const int rc = verify_rows(st, seal_args(p->t, ka.evk, (size_t)p->dnum * 2, ka.M, 0), key.seal_key, key.flags_key, key.part);
    if (rc) return rc;
    e = launch_ks_mac_checked(st, ka, k);
    return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_ks_mac_checked");
}

extern "C" {

int fhe_ctx_inject_fault_keyswitch_sealed(fhe_ctx *ctx, int key_row, long long coeff, int bit)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    return ctx->ks_seal_fault.arm(INT_MAX, key_row, 0, key_row, coeff, bit) ? FHE_OK : fail(FHE_ERR_INVALID, "bad fault");
}

int fhe_keyswitch_sealed_layout(const fhe_keyswitch *p, int out[4])
{
    if (!p || !out) return fail(FHE_ERR_INVALID, "null argument");
    out[0] = 0;
    out[1] = (int)key_rows(p);
    out[2] = out[1] + ksc_layout(p, sealed_form(p).form).total;
    out[3] = ks_sealed_fused(p) ? 1 : 0;
    return FHE_OK;
}

int fhe_keyswitch_apply_sealed(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c, const uint64_t *d_evk,
                               const uint64_t *d_add0, const uint64_t *d_add1, const fhe_abft *a, const uint64_t *d_seal_key, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    const SealedForm f = sealed_form(p);
    const KsForm form = f.form;
    // both hooks belong to this call whatever its outcome
    const StagedFault ft = (ctx->*f.ks_hook).take();
    const SealHook kf = ctx->ks_seal_fault.take();
    int rc = ksc_scope(ctx, p, a, d_flags, form, false);
    if (rc) return rc;
    if (!d_out0 || !d_out1 || !d_c || !d_evk) return fail(FHE_ERR_INVALID, "null argument");
    if (d_out0 == d_out1) return fail(FHE_ERR_INVALID, "the two output parts must be distinct buffers");
    if (misaligned({d_out0, d_out1, d_c, d_evk, d_add0, d_add1})) return fail(FHE_ERR_INVALID, "sealed rows are read 16 bytes at a time: the buffers must be 16-byte aligned");
    SealedKeyStep key{d_seal_key, d_flags, nullptr, KsSealHit{0, 0, 0}};
    if ((rc = ks_seal_hit(kf, p, key.hit))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    // the checked key switch's own hook, against the call: before anything is launched (keyswitch_checked checks it again)
    if ((rc = ksc_prepare(p))) return rc;
    KscHook h;
    if ((rc = ksc_hook(p, form, ft, p->acc.as<u64>(), d_add0 != nullptr, d_add1 != nullptr, h))) return rc;
    int lay[4];
    if ((rc = fhe_keyswitch_sealed_layout(p, lay))) return rc;
    hipStream_t st = pick(ctx, stream);
    if ((rc = seal_scratch(ctx, st, ks_sealed_scratch_words(p), &key.part))) return rc;
    HIP_TRY(hipMemsetAsync(d_flags, 0, (size_t)lay[1] * sizeof(u32), st));
    return keyswitch_checked(p, form, d_out0, d_out1, d_c, d_evk, d_add0, d_add1, a, d_flags + lay[1], st, ft, &key);
}

} // extern "C"
