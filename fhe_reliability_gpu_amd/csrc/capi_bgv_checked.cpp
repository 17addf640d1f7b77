// capi_bgv_checked.cpp -- the BGV forms (plans with a plain modulus t) of the stage-by-stage checked key switch, relinearisation,
// rotation, mod switch and homomorphic multiply, and the checked scalar multiply they are made with (part of the C ABI of
// include/fhe_mi355x.h; shared pieces in capi_checked.hpp).
//
// A BGV mod-down removes t [acc t^-1]_P instead of [acc]_P, a BGV mod switch t [c t^-1]_{q_last} instead of [c]_{q_last}, so that
// what is removed vanishes modulo t.  Next to the CKKS-form launch lists of capi_keyswitch_checked.cpp and capi_hmult_checked.cpp
// that is two word-wise scalar stages each, both in place and both launch_scalar_affine_checked:
//   key switch   9  special limbs of both halves of the sums times t^-1 mod p_k (coefficient form)    between stages 4 and 5
//               10  converted limbs of both halves times t mod q_j (coefficient form)                 between stages 5 and 6
//   mod switch   4  each part's last limb times t^-1 mod q_last (coefficient form)                    between stages 0 and 1
//                5  the residues times t mod q_j                                                      between stages 1 and 2
// The lists themselves are ksc_front / ksc_back and rescale_checked with the BGV hand-over (BgvStages): nothing is copied.  Every
// stage yields canonical residues and those are unique, so the outputs are the unchecked calls' words whichever route those took
// (t riding on the fused tail as RowEpiArgs::pre, or a launch of its own).
// The existing checked calls refuse a plan with a plain modulus and keep doing so; these calls refuse a plan without one.  They
// have hooks of their own (fhe_ctx_inject_fault_bgv_keyswitch / _bgv_mod_switch) and neither take nor honour the others'.
#include "capi_checked.hpp"
#include "keyswitch_check.hpp"
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

namespace {

struct BgvKscLayout {
    KscLayout ks;
    int off9, off10, total;
};
BgvKscLayout bgv_ksc_layout(const fhe_keyswitch *p)
{
    const KscLayout ks = ksc_layout(p);
    return BgvKscLayout{ks, ks.total, ks.total + 2 * p->K, ks.total + 2 * p->K + 2 * p->L};
}

struct BgvRscLayout {
    RscLayout rs;
    int off4, off5, total;
};
BgvRscLayout bgv_rsc_layout(const fhe_keyswitch *p, size_t n_parts)
{
    const RscLayout rs = rsc_layout(p, n_parts);
    const int n = (int)n_parts;
    return BgvRscLayout{rs, rs.total, rs.total + n, rs.total + n + n * (p->L - 1)};
}

int bgv_scope(const fhe_ctx *ctx, const fhe_keyswitch *p, const fhe_abft *a, const uint32_t *d_flags, bool mod_switch)
{
    int rc = ksc_scope(ctx, p, a, d_flags, true);
    if (rc) return rc;
    if (p->L > SCALAR_MAX_LIMBS || p->K > SCALAR_MAX_LIMBS) return fail(FHE_ERR_UNSUPPORTED, "the scalar stages take at most 64 limbs");
    if (mod_switch && p->L < 2) return fail(FHE_ERR_INVALID, "no prime left to drop");
    return FHE_OK;
}

// a fault of one of the two scalar stages, checked against the call: `units` flag words, no addend
int bgv_scalar_fault(const StagedFault &ft, int units, size_t N)
{
    if (ft.unit >= units || (size_t)ft.coeff >= N) return fail(FHE_ERR_INVALID, "fault unit or coefficient outside the call");
    if (!scalar_affine_point_exists(ft.point, false))
        return fail(FHE_ERR_UNSUPPORTED, "fault point 3 (the running sum) does not exist on the BGV scalar stages: they have no addend");
    return FHE_OK;
}

// the two hooks checked against a call, before anything is launched: what the CKKS-form list runs (h / rf) and what the scalar
// stages run (sc, its stage rebased to 0 = times t^-1, 1 = times t)
int bgv_ksc_hook(const fhe_keyswitch *p, const StagedFault &ft, bool has_add0, bool has_add1, KscHook &h, StagedFault &sc)
{
    h = KscHook{};
    sc = StagedFault{};
    if (ft.stage < 9) return ksc_hook(p, ft, p->acc.as<u64>(), has_add0, has_add1, h);
    int rc = bgv_scalar_fault(ft, ft.stage == 9 ? 2 * p->K : 2 * p->L, (size_t)1 << p->log_n);
    if (rc) return rc;
    sc = ft;
    sc.block = 0;
    sc.stage = ft.stage - 9;
    return FHE_OK;
}

int bgv_rsc_hook(const fhe_keyswitch *p, const StagedFault &ft, size_t n_parts, StagedFault &rf, StagedFault &sc)
{
    rf = sc = StagedFault{};
    u64 *flip;
    if (ft.stage < 4) {
        rf = ft;
        return rsc_hook(p, ft, n_parts, &flip);
    }
    int rc = bgv_scalar_fault(ft, ft.stage == 4 ? (int)n_parts : (int)n_parts * (p->L - 1), (size_t)1 << p->log_n);
    if (rc) return rc;
    sc = ft;
    sc.block = 0;
    sc.stage = ft.stage - 4;
    return FHE_OK;
}

// the BGV key switch; the caller has checked scope and arguments.  ft: the fault taken from the BGV key-switch hook
int bgv_keyswitch_checked(fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c, const uint64_t *d_evk, const uint64_t *d_add0,
                          const uint64_t *d_add1, const fhe_abft *a, uint32_t *d_flags, hipStream_t st, const StagedFault &ft)
{
    int rc;
    if ((rc = ksc_prepare(p))) return rc;
    const BgvKscLayout lay = bgv_ksc_layout(p);
    KscHook h;
    BgvStages bgv{d_flags + lay.off9, d_flags + lay.off10, StagedFault{}};
    if ((rc = bgv_ksc_hook(p, ft, d_add0 != nullptr, d_add1 != nullptr, h, bgv.f))) return rc;
    KscFlags fl{};
    for (int s = 0; s < 8; s++) fl.s[s] = d_flags + lay.ks.off[s];
    HIP_TRY(hipMemsetAsync(d_flags, 0, (size_t)lay.total * sizeof(u32), st));
    if ((rc = ksc_front(p, d_c, a, fl, st, h))) return rc;
    return ksc_back(p, d_out0, d_out1, d_c, d_evk, d_add0, d_add1, a, fl, st, h, nullptr, &bgv);
}

// the BGV mod switch; the caller has checked scope, arguments and overlap.  ft: the fault taken from the BGV mod-switch hook
int bgv_mod_switch_checked(fhe_keyswitch *p, uint64_t *const *outs, const uint64_t *d_in, size_t n_parts, const fhe_abft *a, uint32_t *d_flags,
                           hipStream_t st, const StagedFault &ft)
{
    const BgvRscLayout lay = bgv_rsc_layout(p, n_parts);
    BgvStages bgv{d_flags + lay.off4, d_flags + lay.off5, StagedFault{}};
    StagedFault rf;
    int rc = bgv_rsc_hook(p, ft, n_parts, rf, bgv.f);
    if (rc) return rc;
    return rescale_checked(p, outs, d_in, n_parts, a, d_flags, st, rf, &bgv);
}

int key_args(const uint64_t *o0, const uint64_t *o1, std::initializer_list<const void *> need)
{
    for (const void *q : need)
        if (!q) return fail(FHE_ERR_INVALID, "null argument");
    if (!o0 || !o1) return fail(FHE_ERR_INVALID, "null argument");
    if (o0 == o1) return fail(FHE_ERR_INVALID, "the two output parts must be distinct buffers");
    return FHE_OK;
}

} // namespace

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

int fhe_bgv_keyswitch_checked_layout(const fhe_keyswitch *p, int out[12])
{
    if (!p || !out) return fail(FHE_ERR_INVALID, "null argument");
    const BgvKscLayout l = bgv_ksc_layout(p);
    for (int s = 0; s < 8; s++) out[s] = l.ks.off[s];
    out[8] = l.off9;
    out[9] = l.off10;
    out[10] = l.total;
    out[11] = 0;
    return FHE_OK;
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

int fhe_bgv_keyswitch_apply_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c, const uint64_t *d_evk,
                                    const uint64_t *d_add0, const uint64_t *d_add1, const fhe_abft *a, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    const StagedFault ft = ctx->bgv_ksc_fault.take();      // one shot, whatever the outcome
    int rc = bgv_scope(ctx, p, a, d_flags, false);
    if (rc) return rc;
    if ((rc = key_args(d_out0, d_out1, {d_c, d_evk}))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return bgv_keyswitch_checked(p, d_out0, d_out1, d_c, d_evk, d_add0, d_add1, a, d_flags, pick(ctx, stream), ft);
}

int fhe_bgv_relinearize_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_d0, const uint64_t *d_d1,
                                const uint64_t *d_d2, const uint64_t *d_relin_key, const fhe_abft *a, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    const StagedFault ft = ctx->bgv_ksc_fault.take();      // one shot, whatever the outcome
    int rc = bgv_scope(ctx, p, a, d_flags, false);
    if (rc) return rc;
    if ((rc = key_args(d_out0, d_out1, {d_d0, d_d1, d_d2, d_relin_key}))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return bgv_keyswitch_checked(p, d_out0, d_out1, d_d2, d_relin_key, d_d0, d_d1, a, d_flags, pick(ctx, stream), ft);
}

int fhe_bgv_rotate_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1,
                           uint32_t galois_elt, const uint64_t *d_galois_key, const fhe_abft *a, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    const StagedFault ft = ctx->bgv_ksc_fault.take();      // one shot, whatever the outcome
    int rc = bgv_scope(ctx, p, a, d_flags, false);
    if (rc) return rc;
    if ((rc = key_args(d_out0, d_out1, {d_c0, d_c1, d_galois_key}))) return rc;
    if (!(galois_elt & 1)) return fail(FHE_ERR_INVALID, "Galois elements are odd");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    // sigma(c1) and sigma(c0) by one unchecked launch into the plan's buffers, exactly as fhe_rotate_checked does
    const size_t N = (size_t)1 << p->log_n;
    u64 *sig1 = p->rot.as<u64>(), *sig0 = sig1 + (size_t)p->L * N;
    hipError_t e = launch_automorphism_ntt(st, sig1, d_c1, (u32)p->L, p->log_n, galois_elt, sig0, d_c0);
    if (e != hipSuccess) return hip_fail(e, "launch_automorphism_ntt");
    return bgv_keyswitch_checked(p, d_out0, d_out1, sig1, d_galois_key, sig0, nullptr, a, d_flags, st, ft);
}

int fhe_bgv_mod_switch_checked_layout(const fhe_keyswitch *p, size_t n_parts, int out[8])
{
    if (!p || !out) return fail(FHE_ERR_INVALID, "null argument");
    if (n_parts < 1 || n_parts > 3) return fail(FHE_ERR_INVALID, "a ciphertext has 1 to 3 parts");
    if (p->L < 2) return fail(FHE_ERR_INVALID, "no prime left to drop");
    const BgvRscLayout l = bgv_rsc_layout(p, n_parts);
    for (int s = 0; s < 4; s++) out[s] = l.rs.off[s];
    out[4] = l.off4;
    out[5] = l.off5;
    out[6] = l.total;
    out[7] = 0;
    return FHE_OK;
}

int fhe_bgv_mod_switch_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out, const uint64_t *d_in, size_t n_parts, const fhe_abft *a,
                               uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    const StagedFault ft = ctx->bgv_rsc_fault.take();      // one shot, whatever the outcome
    int rc = bgv_scope(ctx, p, a, d_flags, true);
    if (rc) return rc;
    if (!d_out || !d_in) return fail(FHE_ERR_INVALID, "null argument");
    if (n_parts < 1 || n_parts > 3) return fail(FHE_ERR_INVALID, "a ciphertext has 1 to 3 parts");
    // input parts are L rows apart, output parts L - 1: any overlap of the output with the input is refused, as fhe_rescale does
    const size_t N = (size_t)1 << p->log_n, step = (size_t)(p->L - 1) * N;
    if (d_out < d_in + n_parts * p->L * N && d_in < d_out + n_parts * step) return fail(FHE_ERR_INVALID, "rescale is out of place");
    uint64_t *outs[3] = {d_out, d_out + step, d_out + 2 * step};
    HIP_TRY(hipSetDevice(ctx->device));
    return bgv_mod_switch_checked(p, outs, d_in, n_parts, a, d_flags, pick(ctx, stream), ft);
}

int fhe_bgv_hmult_checked_layout(const fhe_keyswitch *p, int rescale, int out[4])
{
    if (!p || !out) return fail(FHE_ERR_INVALID, "null argument");
    if (rescale && p->L < 2) return fail(FHE_ERR_INVALID, "no prime left to drop");
    out[0] = 0;
    out[1] = 3 * p->L;
    out[2] = out[1] + bgv_ksc_layout(p).total;
    out[3] = out[2] + (rescale ? bgv_rsc_layout(p, 2).total : 0);
    return FHE_OK;
}

int fhe_bgv_hmult_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_a0, const uint64_t *d_a1,
                          const uint64_t *d_b0, const uint64_t *d_b1, const uint64_t *d_relin_key, int rescale, const fhe_abft *a, uint32_t *d_flags,
                          void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    // the one-shot hooks of the steps this call runs belong to it whatever its outcome: the BGV key switch's and (when it switches
    // the modulus) the BGV mod switch's are taken here, the pointwise one by the tensor step (cleared here when the call ends before it)
    const StagedFault kf = ctx->bgv_ksc_fault.take(), rf = rescale ? ctx->bgv_rsc_fault.take() : StagedFault{};
    int rc = bgv_scope(ctx, p, a, d_flags, rescale != 0);
    if (!rc) rc = key_args(d_out0, d_out1, {d_a0, d_a1, d_b0, d_b1, d_relin_key});
    if (rc) {
        (void)ctx->pw_fault.take();
        return rc;
    }
    int lay[4];
    const size_t N = (size_t)1 << p->log_n, L = p->L;
    // every hook is checked against the call before the first launch (the steps check them again, to the same end)
    {
        KscHook h;
        StagedFault s0, s1;
        BcCheck k{d_flags, -1, 0, 0, 0};
        if (!(rc = fhe_bgv_hmult_checked_layout(p, rescale, lay)) && !(rc = ksc_prepare(p)) && !(rc = bgv_ksc_hook(p, kf, true, true, h, s0)) &&
            !(rc = rescale ? bgv_rsc_hook(p, rf, 2, s0, s1) : FHE_OK))
            rc = pointwise_fault(ctx->pw_fault, true, L << p->log_n, p->log_n, k);
        if (rc) {
            (void)ctx->pw_fault.take();
            return rc;
        }
    }
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    HIP_TRY(hipMemsetAsync(d_flags, 0, (size_t)lay[3] * sizeof(u32), st));
    u64 *d0 = p->hm.as<u64>(), *d1 = d0 + L * N, *d2 = d1 + L * N, *pre = p->hm_pre.as<u64>();
    if ((rc = fhe_tensor_product_checked(ctx, d0, d1, d2, d_a0, d_a1, d_b0, d_b1, p->t, L, 0, d_flags + lay[0], st))) return rc;
    if (!rescale) return bgv_keyswitch_checked(p, d_out0, d_out1, d2, d_relin_key, d0, d1, a, d_flags + lay[1], st, kf);
    if ((rc = bgv_keyswitch_checked(p, pre, pre + L * N, d2, d_relin_key, d0, d1, a, d_flags + lay[1], st, kf))) return rc;
    uint64_t *outs[3] = {d_out0, d_out1, nullptr};
    return bgv_mod_switch_checked(p, outs, pre, 2, a, d_flags + lay[2], st, rf);
}

} // extern "C"
