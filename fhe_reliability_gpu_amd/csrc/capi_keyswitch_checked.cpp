// capi_keyswitch_checked.cpp -- hybrid key switch, relinearisation and rotation with every stage checked and one flag word per
// (stage, unit) (part of the C ABI of include/fhe_mi355x.h; shared pieces in capi_internal.hpp).
//
// The launch list is the "plain" route of capi_keyswitch.cpp with each launch replaced by its checked form -- none of the unchecked
// call's fusions (k_ks_rowmac, the Galois map and the one-limb conversions riding on loads, the unit-list column pass, the fused
// k_ntt_row_subscale tail):
//   0  copy of d_c into the plan's coefficient buffer, checked INTT of its L limbs in place              (launch_ntt_checked, inverse)
//   1  per digit one checked exact conversion into ext, then one scatter of the flags into limb order    (launch_baseconv_exact_checked)
//   2  checked forward transform of ext: the K special rows of all digits in one launch per run of an arithmetic path, the
//      ciphertext rows per digit and contiguous run of rows (the digit's own limbs are skipped)          (launch_ntt_checked)
//   3  inner product with both key halves                                                                (launch_ks_mac_checked)
//   4  checked INTT of the K special rows of both halves of acc, in place                                (launch_ntt_checked, inverse)
//   5  per half one checked exact conversion P -> Q into conv                                            (launch_baseconv_exact_checked)
//   6  checked forward transform of conv                                                                 (launch_ntt_checked)
//   7  tail (acc - conv) P^-1 (+ addends)                                                                (launch_sub_scale_checked)
// keyswitch_checked = ksc_front (stages 0-2) + ksc_back (stages 3-7); the hoisted rotations of capi_rotate_hoisted_checked.cpp run the
// front once and the back once per Galois element, with the checked Galois permutation between stages 3 and 4.
// The BGV form (plans with a plain modulus t; fhe_bgv_*_checked) removes t [acc t^-1]_P instead of [acc]_P, so that what is removed
// vanishes modulo t: two word-wise scalar stages more, both in place and both launch_scalar_affine_checked (bgv_scalar_stage):
//   9  special limbs of both halves of the sums times t^-1 mod p_k (coefficient form)                    between stages 4 and 5
//  10  converted limbs of both halves times t mod q_j (coefficient form)                                 between stages 5 and 6
// The unchecked call has t riding on the fused tail (RowEpiArgs::pre) or a launch of its own.  The CKKS entry points refuse a
// plan with a plain modulus, the BGV ones a plan without; each form has a hook of its own and neither takes nor honours the other's.
// Each transform stage ends with launch_compare_sums on its units.  Every stage yields canonical residues and canonical residues are
// unique, so the outputs are the unchecked call's words whatever its launch list was.
#include "capi_checked.hpp"
#include "keyswitch_check.hpp"
#include "scalar_check.hpp"

KscLayout ksc_layout(const fhe_keyswitch *p, KsForm form)
{
    const int L = p->L, K = p->K, M = L + K, d = p->dnum, bgv = form == KsForm::BGV;
    const int n[11] = {L, d * M, d * M, 2 * M, 2 * K, 2 * (K + L), 2 * L, 2 * L, 0, bgv * 2 * K, bgv * 2 * L};
    KscLayout l{};
    for (int s = 0; s < 11; s++) {
        l.off[s] = l.total;
        l.total += n[s];
    }
    return l;
}

// the flag map of stage 1, its job-order scratch and the detector's partial sums, once per plan
int ksc_prepare(fhe_keyswitch *p)
{
    if (p->chk_bc_map.p) return FHE_OK;
    u32 tf[2], ti[2];
    ntt_checked_tiles(p->log_n, &tf[0], &tf[1], false);
    ntt_checked_tiles(p->log_n, &ti[0], &ti[1], true);
    const size_t sum_bytes = ksc_slots(p) * 8 * std::max(std::max(tf[0], tf[1]), std::max(ti[0], ti[1]));
    HIP_TRY(p->chk_sum_in.alloc(sum_bytes));
    HIP_TRY(p->chk_sum_out.alloc(sum_bytes));
    const int L = p->L, M = L + p->K;
    std::vector<u32> map((size_t)p->dnum * M);
    for (int d = 0; d < p->dnum; d++) {
        const int lo = d * p->alpha, hi = std::min(L, lo + p->alpha), m = hi - lo;
        for (int j = 0; j < M; j++) {
            const int ju = j >= lo && j < hi ? j - lo : m + (j < lo ? j : j - m);      // unit of limb j in the conversion job's flags
            map[(size_t)d * M + ju] = (u32)(d * M + j);
        }
    }
    HIP_TRY(p->chk_bc_flags.alloc(map.size() * sizeof(u32)));
    HIP_TRY(p->chk_bc_map.upload(map));
    return FHE_OK;
}

// the test hook of one checked key switch, checked against the call before anything is launched: which word a transform stage flips
// between its two launches, which check record a residue stage arms.  acc = the sums stages 4 and 5 work on
int ksc_hook(const fhe_keyswitch *p, KsForm form, const StagedFault &ft, u64 *acc, bool has_add0, bool has_add1, KscHook &h)
{
    const int L = p->L, K = p->K, M = L + K, logn = p->log_n;
    const size_t N = (size_t)1 << logn;
    const KscLayout lay = ksc_layout(p, form);
    u64 *coef = p->coef.as<u64>(), *ext = p->ext.as<u64>(), *conv = p->conv.as<u64>();
    h = KscHook{};
    if (ft.stage < 0) return FHE_OK;
    h.f = ft;
    h.f.block = 0;
    const bool tf = ft.stage < 8 && !(ft.stage & 1);      // a transform stage
    if (ft.unit >= lay.units(ft.stage) || (size_t)ft.coeff >= N) return fail(FHE_ERR_INVALID, "fault unit or coefficient outside the call");
    if (tf && logn < 13) return fail(FHE_ERR_UNSUPPORTED, "the transform stages' fault point lies between their two launches: two-launch sizes only (N >= 2^13)");
    const int u = ft.unit;
    switch (ft.stage) {
    case 0: h.flip = coef + (size_t)u * N + ft.coeff; break;
    case 2: {
        const int d = u / M, j = u % M;
        if (j >= d * p->alpha && j < std::min(L, (d + 1) * p->alpha)) return fail(FHE_ERR_INVALID, "fault unit is one of the digit's own limbs, which stage 2 does not transform");
        h.flip = ext + (size_t)u * N + ft.coeff;
        break;
    }
    case 4: h.flip = acc + ((size_t)(u / K) * M + L + u % K) * N + ft.coeff; break;
    case 6: h.flip = conv + (size_t)u * N + ft.coeff; break;
    case 1: {
        const int d = u / M, j = u % M, lo = d * p->alpha, hi = std::min(L, lo + p->alpha), m = hi - lo;
        const int ju = j >= lo && j < hi ? j - lo : m + (j < lo ? j : j - m);
        if (!bc_point_exists(ft.point, ju < m ? ju + 1 : m))
            return fail(FHE_ERR_UNSUPPORTED, "fault point 3 (the running sum) needs a sum of two terms: not on a digit's first limb, not on a one-limb digit");
        h.f.block = d;
        h.f.unit = ju;
        break;
    }
    case 5: {
        const int ju = u % (K + L);
        if (!bc_point_exists(ft.point, ju < K ? ju + 1 : K))
            return fail(FHE_ERR_UNSUPPORTED, "fault point 3 (the running sum) needs a sum of two terms: not on the first special limb, not with K = 1");
        h.f.block = u / (K + L);
        h.f.unit = ju;
        break;
    }
    case 3:
        if (ft.point < 0 || ft.point > 3) return fail(FHE_ERR_INVALID, "bad fault point");
        break;
    case 7:
        if (!ks_tail_point_exists(ft.point, u / L ? has_add1 : has_add0))
            return fail(FHE_ERR_UNSUPPORTED, "fault point 3 (the running sum) of the tail exists only on a half with an addend");
        break;
    default:      // 9, 10
        if (!scalar_affine_point_exists(ft.point, false))
            return fail(FHE_ERR_UNSUPPORTED, "fault point 3 (the running sum) does not exist on the BGV scalar stages: they have no addend");
        break;
    }
    return FHE_OK;
}

KscNtt ksc_ntt(const fhe_keyswitch *p, const fhe_abft *a, hipStream_t st, bool inverse)
{
    u32 tin, tout;
    ntt_checked_tiles(p->log_n, &tin, &tout, inverse);
    return KscNtt{p, a, st, tin, tout, inverse};
}

// stages 0-2: what does not depend on the key (nor, for hoisted rotations, on the Galois element)
int ksc_front(fhe_keyswitch *p, const uint64_t *d_c, const fhe_abft *a, const KscFlags &fl, hipStream_t st, const KscHook &h, const SealedSteps &steps)
{
    const int L = p->L, K = p->K, M = L + K, dnum = p->dnum;
    const size_t N = (size_t)1 << p->log_n;
    u64 *coef = p->coef.as<u64>(), *ext = p->ext.as<u64>();
    int rc;
    hipError_t e;
    HIP_TRY(hipMemsetAsync(p->chk_bc_flags.p, 0, (size_t)dnum * M * sizeof(u32), st));
    const KscNtt fwd = ksc_ntt(p, a, st, false), inv = ksc_ntt(p, a, st, true);

    // ---- 0: opening INTT (in: no copy, d_c's seal verified on the transform's own load, capi_ntt_sealed.cpp)
    if (steps.in) {
        if ((rc = inv.run_sealed(KscRows{coef, 0, 0, (u32)L, 1, (u32)L, 0}, d_c, *steps.in, h.f.stage == 0 ? h.flip : nullptr, h.f.bit))) return rc;
    } else {
        HIP_TRY(hipMemcpyAsync(coef, d_c, (size_t)L * N * 8, hipMemcpyDeviceToDevice, st));
        if ((rc = inv.run({KscRows{coef, 0, 0, (u32)L, 1, (u32)L, 0}}, h.f.stage == 0 ? h.flip : nullptr, h.f.bit))) return rc;
    }
    if ((rc = inv.compare(fl.s[0], 0, 0, (u32)L, (u32)L))) return rc;

    // ---- 1: digit extension
    for (int d = 0; d < dnum; d++) {
        const BcCheckedJob cj{p->up_host[d], p->up[d]->shoup_dig, p->up[d]->shoup_hor, bc_check(h.f.at(d, 1), p->chk_bc_flags.as<u32>() + (size_t)d * M)};
        if ((e = launch_baseconv_exact_checked(st, cj, N)) != hipSuccess) return hip_fail(e, "launch_baseconv_exact_checked");
    }
    if ((e = launch_ks_flags_scatter(st, fl.s[1], p->chk_bc_flags.as<u32>(), p->chk_bc_map.as<u32>(), (u32)(dnum * M))) != hipSuccess)
        return hip_fail(e, "launch_ks_flags_scatter");

    // ---- 2: forward transform of the extended limbs (the sums of the digits' own limbs stay zero on both sides)
    HIP_TRY(hipMemsetAsync(p->chk_sum_in.p, 0, (size_t)dnum * M * 8 * fwd.tin, st));
    HIP_TRY(hipMemsetAsync(p->chk_sum_out.p, 0, (size_t)dnum * M * 8 * fwd.tout, st));
    std::vector<KscRows> rows;
    rows.push_back(KscRows{ext, (u32)L, (u32)L, (u32)K, (u32)dnum, (u32)M, 0});
    for (int d = 0; d < dnum; d++) {
        const int lo = d * p->alpha, hi = std::min(L, lo + p->alpha);
        u64 *base = ext + (size_t)d * M * N;
        if (lo > 0) rows.push_back(KscRows{base, 0, 0, (u32)lo, 1, (u32)M, (u32)(d * M)});
        if (hi < L) rows.push_back(KscRows{base, (u32)hi, (u32)hi, (u32)(L - hi), 1, (u32)M, (u32)(d * M)});
    }
    if ((rc = fwd.run(rows, h.f.stage == 2 ? h.flip : nullptr, h.f.bit))) return rc;
    return fwd.compare(fl.s[2], 0, 0, (u32)M, (u32)(dnum * M));
}

// stages 3-7 on the digits ksc_front left in the plan.  perm (hoisted rotations): between stages 3 and 4 the sums and perm->c0 go
// through the checked Galois permutation (stage 8, flags fl.s[8]); stages 4-7 then run on the permuted sums with sigma(c0) as d_add0.
// BGV form: the special limbs times t^-1 mod p_k between stages 4 and 5 (stage 9), the converted limbs times t mod q_j between
// stages 5 and 6 (stage 10), so that the part the mod-down removes is t [acc t^-1]_P
int ksc_back(fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c, const uint64_t *d_evk, const uint64_t *d_add0,
             const uint64_t *d_add1, const fhe_abft *a, const KscFlags &fl, hipStream_t st, const KscHook &h, const KscPerm *perm,
             KsForm form, const SealedSteps &steps)
{
    const int L = p->L, K = p->K, M = L + K, logn = p->log_n;
    const size_t N = (size_t)1 << logn;
    const LimbParams *lp = p->t->d_lp.as<LimbParams>();
    u64 *acc = p->acc.as<u64>(), *conv = p->conv.as<u64>();
    int rc;
    hipError_t e;
    const KscNtt fwd = ksc_ntt(p, a, st, false), inv = ksc_ntt(p, a, st, true);
    const bool bgv = form == KsForm::BGV;
    const SealedTailStep *tail = steps.tail;

    // ---- 3: inner product with the key (key: its seal verified on these loads, capi_keyswitch_sealed.cpp)
    {
        const KsMacArgs ka{acc, p->ext.as<u64>(), d_c, d_evk, lp, (u32)L, (u32)M, (u32)p->dnum, (u32)p->alpha, logn, (u32)L, 0u, 0u};
        if (steps.key) {
            if ((rc = ks_mac_sealed_stage(p, st, ka, bc_check(h.f.at(0, 3), fl.s[3]), *steps.key))) return rc;
        } else if ((e = launch_ks_mac_checked(st, ka, bc_check(h.f.at(0, 3), fl.s[3]))) != hipSuccess) return hip_fail(e, "launch_ks_mac_checked");
    }

    // ---- 8: sigma of the sums and of c0
    if (perm) {
        const GalSeg segs[2] = {{perm->acc_to, acc, (u32)(2 * M)}, {perm->c0_to, perm->c0, (u32)L}};
        if ((rc = galois_permute_checked(p->ctx, st, segs, perm->seal_c0 ? 1 : 2, logn, perm->galois_elt, fl.s[8], perm->fault))) return rc;
        if (perm->seal_c0) {
            // c0 verified on the permutation's own gather (galois_sealed.hip); its words of fl.s[8] stay zero
            const GalSealArgs ga{perm->c0_to, perm->c0, lp, 0u, (u32)L, (u32)L, (u32)L, logn, perm->galois_elt};
            if ((e = launch_automorphism_ntt_sealed(st, ga, perm->part, perm->seal_c0, nullptr, perm->flags_c0, perm->hit)) != hipSuccess)
                return hip_fail(e, "launch_automorphism_ntt_sealed");
        }
        acc = perm->acc_to;
        d_add0 = perm->c0_to;
    }

    // ---- 4: INTT of the special limbs of both halves, in place inside the sums
    if ((rc = inv.run({KscRows{acc, (u32)L, (u32)L, (u32)K, 2, (u32)M, 0}}, h.f.stage == 4 ? h.flip : nullptr, h.f.bit))) return rc;
    for (int hf = 0; hf < 2; hf++)
        if ((rc = inv.compare(fl.s[4] + hf * K, (u32)(hf * M + L), (u32)L, (u32)K, (u32)K))) return rc;

    // ---- 9 (BGV): special limbs of both halves times t^-1, in place inside the sums
    if (bgv && (rc = bgv_scalar_stage(p, st, acc + (size_t)L * N, p->t_inv_P.data(), (u32)L, (u32)K, 2, (u32)M, fl.s[9], h.f.at(0, 9)))) return rc;

    // ---- 5: mod-down conversion P -> Q
    for (int hf = 0; hf < 2; hf++) {
        const BcJob job{p->down->dev, acc, conv + (size_t)hf * L * N, 0xFFFFFFFFu, 0u, p->down_rows.as<u32>() + (size_t)hf * K};
        const BcCheckedJob cj{job, p->down->shoup_dig, p->down->shoup_hor, bc_check(h.f.at(hf, 5), fl.s[5] + hf * (K + L))};
        if ((e = launch_baseconv_exact_checked(st, cj, N)) != hipSuccess) return hip_fail(e, "launch_baseconv_exact_checked");
    }

    // ---- 10 (BGV): converted limbs of both halves times t
    if (bgv && (rc = bgv_scalar_stage(p, st, conv, p->t_mod_Q.data(), 0, (u32)L, 2, (u32)L, fl.s[10], h.f.at(0, 10)))) return rc;

    // ---- 6: forward transform of the converted limbs
    if ((rc = fwd.run({KscRows{conv, 0, 0, (u32)L, 2, (u32)L, 0}}, h.f.stage == 6 ? h.flip : nullptr, h.f.bit))) return rc;
    if ((rc = fwd.compare(fl.s[6], 0, 0, (u32)L, (u32)(2 * L)))) return rc;

    // ---- 7: tail (tail: the outputs' seals written from the registers it stores, capi_subscale_sealed.cpp)
    const SubScaleArgs sa{d_out0, d_out1, acc, conv, d_add0, p->pinv.as<u64>(), (u64)((size_t)M * N), (u64)((size_t)L * N), lp, 0u, (u32)L, logn, d_add1};
    if (tail && tail->runs(0, true)) {
        if ((e = launch_sub_scale_sealed(st, sa, bc_check(h.f.at(0, 7), fl.s[7]), tail->launch(0, true, (u32)L, 0))) != hipSuccess)
            return hip_fail(e, "launch_sub_scale_sealed");
    } else if ((e = launch_sub_scale_checked(st, sa, bc_check(h.f.at(0, 7), fl.s[7]))) != hipSuccess) return hip_fail(e, "launch_sub_scale_checked");
    return FHE_OK;
}

int keyswitch_checked(fhe_keyswitch *p, KsForm form, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c, const uint64_t *d_evk,
                      const uint64_t *d_add0, const uint64_t *d_add1, const fhe_abft *a, uint32_t *d_flags, hipStream_t st, const StagedFault &ft,
                      const SealedSteps &steps)
{
    int rc;
    if ((rc = ksc_prepare(p))) return rc;
    KscHook h;
    if ((rc = ksc_hook(p, form, ft, p->acc.as<u64>(), d_add0 != nullptr, d_add1 != nullptr, h))) return rc;
    const KscLayout lay = ksc_layout(p, form);
    KscFlags fl{};
    for (int s = 0; s < 11; s++)
        if (lay.units(s)) fl.s[s] = d_flags + lay.off[s];
    HIP_TRY(hipMemsetAsync(d_flags, 0, (size_t)lay.total * sizeof(u32), st));
    if ((rc = ksc_front(p, d_c, a, fl, st, h, steps))) return rc;
    return ksc_back(p, d_out0, d_out1, d_c, d_evk, d_add0, d_add1, a, fl, st, h, nullptr, form, steps);
}

int ksc_scope(const fhe_ctx *ctx, const fhe_keyswitch *p, const fhe_abft *a, const uint32_t *d_flags, KsForm form, bool mod_switch)
{
    const bool bgv = form == KsForm::BGV;
    if (!p || !a || !d_flags) return fail(FHE_ERR_INVALID, "null argument");
    if (a->t != p->t) return fail(FHE_ERR_INVALID, "the detector was made for another table set than the plan's");
    if (p->sharded) return fail(FHE_ERR_INVALID, "a sharded plan has no checked key switch: the checked call runs the whole switch on one device");
    if (!bgv && p->plain_modulus) return fail(FHE_ERR_UNSUPPORTED, "the BGV steps of a plan with a plain modulus have no checked form");
    if (bgv && !p->plain_modulus) return fail(FHE_ERR_INVALID, "the plan has no plain modulus: use the existing checked calls");
    if (int rc = ksc_rounding_scope(p, mod_switch)) return rc;      // (after the form: a BGV-form call on a plan without a plain modulus answers as it did)
    if (ctx->mode != 0 || ctx->resident || ctx->packed_on || ctx->only_pass >= 0 || !ntt_checked_supported(p->log_n))
        return fail(FHE_ERR_UNSUPPORTED, "the checked key switch runs the two-launch transforms: not with ntt_mode=1, ntt_resident, ntt_packed, a single-pass hook, or N < 2^5");
    if (!p->t->has_inverse) return fail(FHE_ERR_UNSUPPORTED, "table set has no inverse (twiddle or N not invertible)");
    if (bgv && (p->L > SCALAR_MAX_LIMBS || p->K > SCALAR_MAX_LIMBS)) return fail(FHE_ERR_UNSUPPORTED, "the scalar stages take at most 64 limbs");
    if (mod_switch && p->L < 2) return fail(FHE_ERR_INVALID, "no prime left to drop");
    return FHE_OK;
}

namespace {

int layout_call(const fhe_keyswitch *p, KsForm form, int *out)
{
    if (!p || !out) return fail(FHE_ERR_INVALID, "null argument");
    const KscLayout l = ksc_layout(p, form);
    int n = 0;
    for (int s = 0; s < 11; s++)
        if (s < 8 || l.units(s)) out[n++] = l.off[s];
    out[n++] = l.total;
    out[n] = 0;
    return FHE_OK;
}

// apply, and relinearisation (need_add: d_d0 and d_d1 are its addends, d_d2 what is switched)
int apply_checked(KsForm form, KsHookSlot hook, fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c,
                  const uint64_t *d_evk, const uint64_t *d_add0, const uint64_t *d_add1, bool need_add, const fhe_abft *a, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    const StagedFault ft = (ctx->*hook).take();      // one shot, whatever the outcome
    int rc = ksc_scope(ctx, p, a, d_flags, form, false);
    if (rc) return rc;
    if (!d_out0 || !d_out1 || !d_c || !d_evk || (need_add && (!d_add0 || !d_add1))) return fail(FHE_ERR_INVALID, "null argument");
    if (d_out0 == d_out1) return fail(FHE_ERR_INVALID, "the two output parts must be distinct buffers");
    HIP_TRY(hipSetDevice(ctx->device));
    return keyswitch_checked(p, form, d_out0, d_out1, d_c, d_evk, d_add0, d_add1, a, d_flags, pick(ctx, stream), ft);
}

} // namespace

int rotate_checked(KsForm form, const StagedFault &ft, fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0,
                   const uint64_t *d_c1, uint32_t galois_elt, const uint64_t *d_galois_key, const fhe_abft *a, uint32_t *d_flags, void *stream,
                   const SealedSteps &steps)
{
    int rc = ksc_scope(ctx, p, a, d_flags, form, false);
    if (rc) return rc;
    if (!d_out0 || !d_out1 || !d_c0 || !d_c1 || !d_galois_key) return fail(FHE_ERR_INVALID, "null argument");
    if (d_out0 == d_out1) return fail(FHE_ERR_INVALID, "the two output parts must be distinct buffers");
    if (!(galois_elt & 1)) return fail(FHE_ERR_INVALID, "Galois elements are odd");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    // sigma(c1) and sigma(c0) (NTT domain: permutations of the slots) by one launch into the plan's buffers; the permutation itself is
    // not checked.  sigma(c1) is switched back to s with the Galois key, sigma(c0) is the first part's addend.
    const size_t N = (size_t)1 << p->log_n;
    u64 *sig1 = p->rot.as<u64>(), *sig0 = sig1 + (size_t)p->L * N;
    hipError_t e = launch_automorphism_ntt(st, sig1, d_c1, (u32)p->L, p->log_n, galois_elt, sig0, d_c0);
    if (e != hipSuccess) return hip_fail(e, "launch_automorphism_ntt");
    return keyswitch_checked(p, form, d_out0, d_out1, sig1, d_galois_key, sig0, nullptr, a, d_flags, st, ft, steps);
}

extern "C" {

int fhe_keyswitch_checked_layout(const fhe_keyswitch *p, int out[10]) { return layout_call(p, KsForm::CKKS, out); }
int fhe_bgv_keyswitch_checked_layout(const fhe_keyswitch *p, int out[12]) { return layout_call(p, KsForm::BGV, out); }

int fhe_ctx_inject_fault_keyswitch(fhe_ctx *ctx, int stage, int point, int unit, long long coeff, int bit)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    return ctx->ksc_fault.arm(KSC_RULES, 0, stage, point, unit, coeff, bit) ? FHE_OK : fail(FHE_ERR_INVALID, "bad fault");
}

int fhe_keyswitch_apply_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c, const uint64_t *d_evk,
                                const uint64_t *d_add0, const uint64_t *d_add1, const fhe_abft *a, uint32_t *d_flags, void *stream)
{
    return apply_checked(KsForm::CKKS, &fhe_ctx::ksc_fault, ctx, p, d_out0, d_out1, d_c, d_evk, d_add0, d_add1, false, a, d_flags, stream);
}

int fhe_bgv_keyswitch_apply_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c, const uint64_t *d_evk,
                                    const uint64_t *d_add0, const uint64_t *d_add1, const fhe_abft *a, uint32_t *d_flags, void *stream)
{
    return apply_checked(KsForm::BGV, &fhe_ctx::bgv_ksc_fault, ctx, p, d_out0, d_out1, d_c, d_evk, d_add0, d_add1, false, a, d_flags, stream);
}

int fhe_relinearize_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_d0, const uint64_t *d_d1,
                            const uint64_t *d_d2, const uint64_t *d_relin_key, const fhe_abft *a, uint32_t *d_flags, void *stream)
{
    return apply_checked(KsForm::CKKS, &fhe_ctx::ksc_fault, ctx, p, d_out0, d_out1, d_d2, d_relin_key, d_d0, d_d1, true, a, d_flags, stream);
}

int fhe_bgv_relinearize_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_d0, const uint64_t *d_d1,
                                const uint64_t *d_d2, const uint64_t *d_relin_key, const fhe_abft *a, uint32_t *d_flags, void *stream)
{
    return apply_checked(KsForm::BGV, &fhe_ctx::bgv_ksc_fault, ctx, p, d_out0, d_out1, d_d2, d_relin_key, d_d0, d_d1, true, a, d_flags, stream);
}

int fhe_rotate_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1,
                       uint32_t galois_elt, const uint64_t *d_galois_key, const fhe_abft *a, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    return rotate_checked(KsForm::CKKS, ctx->ksc_fault.take(), ctx, p, d_out0, d_out1, d_c0, d_c1, galois_elt, d_galois_key, a, d_flags, stream);
}

int fhe_bgv_rotate_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1,
                           uint32_t galois_elt, const uint64_t *d_galois_key, const fhe_abft *a, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    return rotate_checked(KsForm::BGV, ctx->bgv_ksc_fault.take(), ctx, p, d_out0, d_out1, d_c0, d_c1, galois_elt, d_galois_key, a, d_flags, stream);
}

} // extern "C"
