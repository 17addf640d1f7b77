// capi_hmult_checked.cpp -- rescale and homomorphic multiply with every stage checked and one flag word per (stage, unit)
// (part of the C ABI of include/fhe_mi355x.h; shared pieces in capi_checked.hpp).
//
// The checked rescale is the "plain" route of capi_hmult.cpp with each launch replaced by its checked form -- neither x mod q_j
// riding on the residues' column pass nor the fused k_ntt_row_subscale tail:
//   0  copy of each part's last limb into the plan's rs_bc, checked INTT in place                (launch_ntt_checked, inverse)
//   1  delta_j = x mod q_j for every remaining prime                                              (launch_rescale_reduce_checked)
//   2  checked forward transform of the residues                                                  (launch_ntt_checked)
//   3  (c - delta) q_last^-1                                                                      (launch_sub_scale_checked)
// Each transform stage ends with launch_compare_sums on its units.  Every stage yields canonical residues and those are unique,
// so the outputs are fhe_rescale's words whichever route it took.  The checked homomorphic multiply is fhe_tensor_product_checked,
// the checked relinearisation and this rescale in a row: fhe_hmult's words whether or not it fused the mod-down with the rescale.
// The BGV form (plans with a plain modulus t; fhe_bgv_mod_switch_checked, fhe_bgv_hmult_checked) removes t [c t^-1]_{q_last}
// instead of [c]_{q_last}: two word-wise scalar stages more, both in place and both launch_scalar_affine_checked (bgv_scalar_stage):
//   4  each part's last limb times t^-1 mod q_last (coefficient form)                             between stages 0 and 1
//   5  the residues times t mod q_j                                                               between stages 1 and 2
// Both forms of the multiply check every hook (pointwise, key switch, rescale) against the call before the first launch: on a
// refusal nothing is enqueued, the flag buffer is untouched and the pointwise hook is cleared.  (fhe_hmult_checked used to run
// the tensor step and the key switch before it refused a bad rescale hook; that is the one behaviour the two forms did not share.)
#include "capi_checked.hpp"
#include "keyswitch_check.hpp"
#include "rescale_check.hpp"
#include "scalar_check.hpp"

RscLayout rsc_layout(const fhe_keyswitch *p, size_t n_parts, KsForm form)
{
    const int n = (int)n_parts, R = p->L - 1, bgv = form == KsForm::BGV;
    const int w[6] = {n, n * R, n * R, n * R, bgv * n, bgv * n * R};
    RscLayout l{};
    for (int s = 0; s < 6; s++) {
        l.off[s] = l.total;
        l.total += w[s];
    }
    return l;
}

// the test hook of one checked rescale, checked against the call before anything is launched; *flip = the word a transform stage
// flips between its two launches
int rsc_hook(const fhe_keyswitch *p, KsForm form, const StagedFault &ft, size_t n_parts, u64 **flip)
{
    const RscLayout lay = rsc_layout(p, n_parts, form);
    const int logn = p->log_n;
    const size_t N = (size_t)1 << logn;
    *flip = nullptr;
    if (ft.stage >= 0) {
        if (ft.unit >= lay.units(ft.stage) || (size_t)ft.coeff >= N) return fail(FHE_ERR_INVALID, "fault unit or coefficient outside the call");
        if (ft.stage >= 4) {
            if (!scalar_affine_point_exists(ft.point, false))
                return fail(FHE_ERR_UNSUPPORTED, "fault point 3 (the running sum) does not exist on the BGV scalar stages: they have no addend");
        } else if (!(ft.stage & 1)) {
            if (logn < 13) return fail(FHE_ERR_UNSUPPORTED, "the transform stages' fault point lies between their two launches: two-launch sizes only (N >= 2^13)");
            *flip = (ft.stage == 0 ? p->rs_bc : p->rs_delta.as<u64>()) + (size_t)ft.unit * N + ft.coeff;
        } else {
            if (ft.stage == 1 && !rescale_reduce_point_exists(ft.point))
                return fail(FHE_ERR_UNSUPPORTED, "fault point 3 (the running sum) does not exist on the rescale's residues: x mod q_j has no sum");
            if (ft.stage == 3 && !ks_tail_point_exists(ft.point, false))
                return fail(FHE_ERR_UNSUPPORTED, "fault point 3 (the running sum) of the tail exists only with an addend, and the rescale has none");
        }
    }
    return FHE_OK;
}

// BGV form: the last limbs times t^-1 mod q_last between stages 0 and 1 (stage 4), the residues times t mod q_j between stages 1
// and 2 (stage 5), so that the part the switch removes is t [c t^-1]_{q_last}
int rescale_checked(fhe_keyswitch *p, KsForm form, uint64_t *const *outs, const uint64_t *d_in, size_t n_parts, const fhe_abft *a, uint32_t *d_flags,
                    hipStream_t st, const StagedFault &ft, const SealedTailStep *tail)
{
    const fhe_ntt_tables *t = p->t;
    const int L = p->L, R = L - 1, logn = p->log_n;
    const size_t N = (size_t)1 << logn;
    const RscLayout lay = rsc_layout(p, n_parts, form);
    const bool bgv = form == KsForm::BGV;
    const LimbParams *lp = t->d_lp.as<LimbParams>();
    u64 *x = p->rs_bc, *delta = p->rs_delta.as<u64>();
    int rc;
    hipError_t e;
    if ((rc = ksc_prepare(p))) return rc;

    // ---- the test hook, checked against this call before anything is launched
    u64 *flip;
    if ((rc = rsc_hook(p, form, ft, n_parts, &flip))) return rc;

    HIP_TRY(hipMemsetAsync(d_flags, 0, (size_t)lay.total * sizeof(u32), st));
    const KscNtt fwd = ksc_ntt(p, a, st, false), inv = ksc_ntt(p, a, st, true);

    // ---- 0: INTT of the last limbs (sealed input: no copy, each part's last limb verified on the transform's own load -- the
    // launcher takes contiguous rows, so one call per part)
    if (tail && tail->flags_in) {
        for (size_t part = 0; part < n_parts; part++) {
            const size_t row = part * L + R;
            SealedInputStep in{tail->seal_in ? tail->seal_in + 2 * row : nullptr, tail->flags_in + row, tail->part_ntt + part * ntt_seal_part_words(1, logn, true), 0, 0, 0};
            if (tail->ntt_hit_part == (int)part) in.hit_coeff = tail->ntt_hit_coeff, in.hit_mask = tail->ntt_hit_mask;
            const bool mine = ft.stage == 0 && (size_t)ft.unit == part;
            if ((rc = inv.run_sealed(KscRows{x + part * N, 0, (u32)R, 1, 1, 1, (u32)part}, d_in + row * N, in, mine ? flip : nullptr, ft.bit))) return rc;
        }
    } else {
        HIP_TRY(hipMemcpy2DAsync(x, N * 8, d_in + (size_t)R * N, (size_t)L * N * 8, N * 8, n_parts, hipMemcpyDeviceToDevice, st));
        if ((rc = inv.run({KscRows{x, 0, (u32)R, 1, (u32)n_parts, 1, 0}}, ft.stage == 0 ? flip : nullptr, ft.bit))) return rc;
    }
    if ((rc = inv.compare(d_flags + lay.off[0], 0, (u32)R, 1, (u32)n_parts))) return rc;

    // ---- 4 (BGV): last limbs times t^-1
    if (bgv && (rc = bgv_scalar_stage(p, st, x, &p->t_inv_qlast, (u32)R, 1, (u32)n_parts, 1, d_flags + lay.off[4], ft.at(0, 4)))) return rc;

    // ---- 1: residues modulo the remaining primes
    const RescaleReduceArgs ra{delta, x, lp, (u32)R, (u32)n_parts, logn};
    if ((e = launch_rescale_reduce_checked(st, ra, bc_check(ft.at(0, 1), d_flags + lay.off[1]))) != hipSuccess) return hip_fail(e, "launch_rescale_reduce_checked");

    // ---- 5 (BGV): residues times t
    if (bgv && (rc = bgv_scalar_stage(p, st, delta, p->t_mod_Q.data(), 0, (u32)R, (u32)n_parts, (u32)R, d_flags + lay.off[5], ft.at(0, 5)))) return rc;

    // ---- 2: forward transform of the residues
    if ((rc = fwd.run({KscRows{delta, 0, 0, (u32)R, (u32)n_parts, (u32)R, 0}}, ft.stage == 2 ? flip : nullptr, ft.bit))) return rc;
    if ((rc = fwd.compare(d_flags + lay.off[2], 0, 0, (u32)R, (u32)(n_parts * R)))) return rc;

    // ---- 3: (c - delta) / q_last, two parts per launch
    for (size_t part = 0; part < n_parts; part += 2) {
        const bool two = part + 1 < n_parts;
        const int u0 = (int)part * R, u1 = u0 + (two ? 2 : 1) * R;
        const BcCheck k = bc_check(ft.at(0, 3), d_flags + lay.off[3] + u0, u0, u1);
        const SubScaleArgs sa{outs[part], two ? outs[part + 1] : nullptr, d_in + part * L * N, delta + part * R * N, nullptr, p->qlast_inv.as<u64>(),
                              (u64)((size_t)L * N), (u64)((size_t)R * N), lp, 0u, (u32)R, logn, nullptr};
        if (tail && tail->runs(part, two)) {
            // the sealed tail: rows 0 .. L - 2 of the parts verified on this load (sealed input), the outputs' seals from the stored registers
            if ((e = launch_sub_scale_sealed(st, sa, k, tail->launch(part, two, (u32)R, (u32)L))) != hipSuccess) return hip_fail(e, "launch_sub_scale_sealed");
        } else if ((e = launch_sub_scale_checked(st, sa, k)) != hipSuccess) return hip_fail(e, "launch_sub_scale_checked");
    }
    return FHE_OK;
}

int hmult_checked_layout(const fhe_keyswitch *p, KsForm form, int rescale, int out[4])
{
    if (!p || !out) return fail(FHE_ERR_INVALID, "null argument");
    if (rescale && p->L < 2) return fail(FHE_ERR_INVALID, "no prime left to drop");
    out[0] = 0;
    out[1] = 3 * p->L;
    out[2] = out[1] + ksc_layout(p, form).total;
    out[3] = out[2] + (rescale ? rsc_layout(p, 2, form).total : 0);
    return FHE_OK;
}

namespace {

int rescale_layout_call(const fhe_keyswitch *p, KsForm form, size_t n_parts, int *out)
{
    if (!p || !out) return fail(FHE_ERR_INVALID, "null argument");
    if (n_parts < 1 || n_parts > 3) return fail(FHE_ERR_INVALID, "a ciphertext has 1 to 3 parts");
    if (p->L < 2) return fail(FHE_ERR_INVALID, "no prime left to drop");
    const RscLayout l = rsc_layout(p, n_parts, form);
    const int stages = form == KsForm::BGV ? 6 : 4;
    for (int s = 0; s < stages; s++) out[s] = l.off[s];
    out[stages] = l.total;
    out[stages + 1] = 0;
    return FHE_OK;
}

int rescale_call(KsForm form, KsHookSlot hook, fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out, const uint64_t *d_in, size_t n_parts, const fhe_abft *a,
                 uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    const StagedFault ft = (ctx->*hook).take();      // one shot, whatever the outcome
    int rc = ksc_scope(ctx, p, a, d_flags, form, true);
    if (rc) return rc;
    if (!d_out || !d_in) return fail(FHE_ERR_INVALID, "null argument");
    if (n_parts < 1 || n_parts > 3) return fail(FHE_ERR_INVALID, "a ciphertext has 1 to 3 parts");
    // input parts are L rows apart, output parts L - 1: any overlap of the output with the input is refused, as fhe_rescale does
    const size_t N = (size_t)1 << p->log_n, step = (size_t)(p->L - 1) * N;
    if (d_out < d_in + n_parts * p->L * N && d_in < d_out + n_parts * step) return fail(FHE_ERR_INVALID, "rescale is out of place");
    uint64_t *outs[3] = {d_out, d_out + step, d_out + 2 * step};
    HIP_TRY(hipSetDevice(ctx->device));
    return rescale_checked(p, form, outs, d_in, n_parts, a, d_flags, pick(ctx, stream), ft);
}

// scope, arguments and every hook of one multiply, checked against the call before its first launch (the steps check their hooks
// again, to the same end)
int hmult_validate(KsForm form, fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_a0, const uint64_t *d_a1,
                   const uint64_t *d_b0, const uint64_t *d_b1, const uint64_t *d_relin_key, int rescale, const fhe_abft *a, uint32_t *d_flags,
                   const HmultHooks &hk, int lay[4])
{
    int rc = ksc_scope(ctx, p, a, d_flags, form, rescale != 0);
    if (rc) return rc;
    if (!d_out0 || !d_out1 || !d_a0 || !d_a1 || !d_b0 || !d_b1 || !d_relin_key) return fail(FHE_ERR_INVALID, "null argument");
    if (d_out0 == d_out1) return fail(FHE_ERR_INVALID, "the two output parts must be distinct buffers");
    if ((rc = hmult_checked_layout(p, form, rescale, lay))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = ksc_prepare(p))) return rc;
    KscHook h;
    u64 *flip;
    BcCheck k{d_flags, -1, 0, 0, 0};
    if ((rc = ksc_hook(p, form, hk.ks, p->acc.as<u64>(), true, true, h))) return rc;
    if (rescale && (rc = rsc_hook(p, form, hk.rs, 2, &flip))) return rc;
    return pointwise_fault(hk.pw, true, (size_t)p->L << p->log_n, p->log_n, k);
}

} // namespace

HmultHooks hmult_take(fhe_ctx *ctx, KsHookSlot ks_hook, KsHookSlot rs_hook, int rescale, bool sealed_tensor)
{
    return HmultHooks{(ctx->*ks_hook).take(), rescale ? (ctx->*rs_hook).take() : StagedFault{}, ctx->pw_fault.take(),
                      sealed_tensor ? ctx->tensor_seal_fault.take() : SealHook{}};
}

int hmult_checked(KsForm form, const HmultHooks &hk, fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_a0,
                  const uint64_t *d_a1, const uint64_t *d_b0, const uint64_t *d_b1, const uint64_t *d_relin_key, int rescale, const fhe_abft *a,
                  uint32_t *d_flags, void *stream, const SealedSteps &steps)
{
    int lay[4];
    int rc = hmult_validate(form, ctx, p, d_out0, d_out1, d_a0, d_a1, d_b0, d_b1, d_relin_key, rescale, a, d_flags, hk, lay);
    TensorSealHit hit{-1, 0, 0, 0};
    if (!rc && steps.tensor) rc = tensor_seal_hit(hk.tensor, (size_t)p->L, p->log_n, hit);
    if (rc) return rc;
    hipStream_t st = pick(ctx, stream);
    HIP_TRY(hipMemsetAsync(d_flags, 0, (size_t)lay[3] * sizeof(u32), st));
    const size_t N = (size_t)1 << p->log_n, L = p->L;
    u64 *d0 = p->hm.as<u64>(), *d1 = d0 + L * N, *d2 = d1 + L * N, *pre = p->hm_pre.as<u64>();
    // (the operands are read by the first step only, the outputs written by the last launches of the last step: an output may reuse
    // an operand's buffer, as for fhe_hmult)
    BcCheck k{d_flags + lay[0], -1, 0, 0, 0};
    if ((rc = pointwise_fault(hk.pw, true, L << p->log_n, p->log_n, k))) return rc;      // validated above
    if (steps.tensor) {
        uint64_t *const d[3] = {d0, d1, d2};
        const uint64_t *const ops[4] = {d_a0, d_a1, d_b0, d_b1};
        if ((rc = tensor_sealed_run(ctx, st, d, ops, p->t, 1, L, 0, steps.tensor->seal_in, nullptr, steps.tensor->flags_op, k, hit))) return rc;
    } else {
        // fhe_tensor_product_checked's launches, with the hook this call took
        HIP_TRY(hipMemsetAsync(k.flags, 0, L * 3 * sizeof(u32), st));
        const TensorArgs ta{d0, d1, d2, d_a0, d_a1, d_b0, d_b1, p->t->d_lp.as<LimbParams>(), 0u, (u32)L, p->log_n};
        hipError_t e = launch_tensor_checked(st, ta, k);
        if (e != hipSuccess) return hip_fail(e, "launch_tensor_checked");
    }
    // (tail: the last launch -- the key switch's stage 7, or with a rescale its stage 3 -- writes the outputs' seals)
    SealedSteps ks;
    ks.key = steps.key;
    if (!rescale) {
        ks.tail = steps.tail;
        return keyswitch_checked(p, form, d_out0, d_out1, d2, d_relin_key, d0, d1, a, d_flags + lay[1], st, hk.ks, ks);
    }
    if ((rc = keyswitch_checked(p, form, pre, pre + L * N, d2, d_relin_key, d0, d1, a, d_flags + lay[1], st, hk.ks, ks))) return rc;
    uint64_t *outs[3] = {d_out0, d_out1, nullptr};
    return rescale_checked(p, form, outs, pre, 2, a, d_flags + lay[2], st, hk.rs, steps.tail);
}

extern "C" {

int fhe_rescale_checked_layout(const fhe_keyswitch *p, size_t n_parts, int out[6]) { return rescale_layout_call(p, KsForm::CKKS, n_parts, out); }
int fhe_bgv_mod_switch_checked_layout(const fhe_keyswitch *p, size_t n_parts, int out[8]) { return rescale_layout_call(p, KsForm::BGV, n_parts, out); }

int fhe_ctx_inject_fault_rescale(fhe_ctx *ctx, int stage, int point, int unit, long long coeff, int bit)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    return ctx->rsc_fault.arm(RSC_RULES, 0, stage, point, unit, coeff, bit) ? FHE_OK : fail(FHE_ERR_INVALID, "bad fault");
}

int fhe_rescale_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out, const uint64_t *d_in, size_t n_parts, const fhe_abft *a, uint32_t *d_flags,
                        void *stream)
{
    return rescale_call(KsForm::CKKS, &fhe_ctx::rsc_fault, ctx, p, d_out, d_in, n_parts, a, d_flags, stream);
}

int fhe_bgv_mod_switch_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out, const uint64_t *d_in, size_t n_parts, const fhe_abft *a,
                               uint32_t *d_flags, void *stream)
{
    return rescale_call(KsForm::BGV, &fhe_ctx::bgv_rsc_fault, ctx, p, d_out, d_in, n_parts, a, d_flags, stream);
}

int fhe_hmult_checked_layout(const fhe_keyswitch *p, int rescale, int out[4]) { return hmult_checked_layout(p, KsForm::CKKS, rescale, out); }
int fhe_bgv_hmult_checked_layout(const fhe_keyswitch *p, int rescale, int out[4]) { return hmult_checked_layout(p, KsForm::BGV, rescale, out); }

int fhe_hmult_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_a0, const uint64_t *d_a1,
                      const uint64_t *d_b0, const uint64_t *d_b1, const uint64_t *d_relin_key, int rescale, const fhe_abft *a, uint32_t *d_flags,
                      void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    return hmult_checked(KsForm::CKKS, hmult_take(ctx, &fhe_ctx::ksc_fault, &fhe_ctx::rsc_fault, rescale, false), ctx, p, d_out0, d_out1, d_a0, d_a1, d_b0, d_b1,
                         d_relin_key, rescale, a, d_flags, stream);
}

int fhe_bgv_hmult_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_a0, const uint64_t *d_a1,
                          const uint64_t *d_b0, const uint64_t *d_b1, const uint64_t *d_relin_key, int rescale, const fhe_abft *a, uint32_t *d_flags,
                          void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    return hmult_checked(KsForm::BGV, hmult_take(ctx, &fhe_ctx::bgv_ksc_fault, &fhe_ctx::bgv_rsc_fault, rescale, false), ctx, p, d_out0, d_out1, d_a0, d_a1, d_b0,
                         d_b1, d_relin_key, rescale, a, d_flags, stream);
}

} // extern "C"
