// capi_bgv_checked.cpp -- the checked scalar multiply (fhe_scalar_affine_checked), the scalar stage the BGV forms of the checked
// composites are made with, and the setters of the BGV forms' hooks (part of the C ABI of include/fhe_mi355x.h; shared pieces in
// capi_checked.hpp).  The BGV forms themselves live with the composites: capi_keyswitch_checked.cpp, capi_hmult_checked.cpp.
#include "capi_checked.hpp"
#include "scalar_check.hpp"

int bgv_scalar_stage(const fhe_keyswitch *p, hipStream_t st, u64 *data, const u64 *scal, u32 limb0, u32 limbs, u32 n_poly, u32 poly_stride, u32 *flags,
                     const StagedFault &f)
{
    if (limbs > (u32)SCALAR_MAX_LIMBS) return fail(FHE_ERR_UNSUPPORTED, "at most 64 limbs per scalar stage");
    ScalarVec m{};
    for (u32 l = 0; l < limbs; l++) m.v[l] = scal[l];      // reduced when the plain modulus was set
    const PointwiseArgs pa{data, data, data, p->t->d_lp.as<LimbParams>(), limb0, limbs, n_poly * limbs, poly_stride, p->log_n};
    hipError_t e = launch_scalar_affine_checked(st, pa, m, nullptr, bc_check(f, flags));
    return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_scalar_affine_checked");
}

extern "C" {

int fhe_scalar_affine_checked(fhe_ctx *ctx, uint64_t *d_c, const uint64_t *d_a, const uint64_t *mul, const uint64_t *add, const fhe_ntt_tables *t,
                              size_t n_poly, size_t limbs, size_t start_idx, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    // the one-shot pointwise hook belongs to this call whatever its outcome
    const PointFault f = ctx->pw_fault.take();
    if (!d_c || !d_a || !d_flags) return fail(FHE_ERR_INVALID, "null argument");
    if (limbs > SCALAR_MAX_LIMBS) return fail(FHE_ERR_UNSUPPORTED, "at most 64 limbs per scalar call");
    int rc = check_range(t, n_poly, limbs, start_idx);
    if (rc) return rc;
    const size_t units = n_poly * limbs;
    if (f.point >= 0 && !scalar_affine_point_exists(f.point, add != nullptr))
        return fail(FHE_ERR_UNSUPPORTED, "fault point 3 (the sum before the conditional subtraction) exists only with an addend");
    BcCheck k{d_flags, -1, 0, 0, 0};
    if ((rc = pointwise_fault(f, true, units << t->log_n, t->log_n, k))) return rc;
    if (!units) return FHE_OK;
    ScalarVec m{}, ad{};
    for (size_t l = 0; l < limbs; l++) {
        const u64 q = t->q[start_idx + l];
        m.v[l] = mul ? mul[l] % q : 1 % q;
        ad.v[l] = add ? add[l] % q : 0;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    HIP_TRY(hipMemsetAsync(d_flags, 0, units * sizeof(u32), st));
    const PointwiseArgs pa{d_c, d_a, d_a, t->d_lp.as<LimbParams>(), (u32)start_idx, (u32)limbs, (u32)units, (u32)limbs, t->log_n};
    hipError_t e = launch_scalar_affine_checked(st, pa, m, add ? &ad : nullptr, k);
    return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_scalar_affine_checked");
}

int fhe_ctx_inject_fault_bgv_keyswitch(fhe_ctx *ctx, int stage, int point, int unit, long long coeff, int bit)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    return ctx->bgv_ksc_fault.arm(BGV_KSC_RULES, 0, stage, point, unit, coeff, bit) ? FHE_OK : fail(FHE_ERR_INVALID, "bad fault");
}

int fhe_ctx_inject_fault_bgv_mod_switch(fhe_ctx *ctx, int stage, int point, int unit, long long coeff, int bit)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    return ctx->bgv_rsc_fault.arm(BGV_RSC_RULES, 0, stage, point, unit, coeff, bit) ? FHE_OK : fail(FHE_ERR_INVALID, "bad fault");
}

} // extern "C"
