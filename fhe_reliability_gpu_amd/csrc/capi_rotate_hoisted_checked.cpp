// capi_rotate_hoisted_checked.cpp -- the checked NTT-domain Galois permutation and hoisted rotations with every stage checked
// (part of the C ABI of include/fhe_mi355x.h; shared pieces in capi_checked.hpp).
//
// Hoisted rotations of one ciphertext by several Galois elements: sigma is a ring automorphism and the prepared keys are in the
// un-rotated frame (fhe_galois_key_prepare), so the decomposition of c1 does not depend on the element.  The launch list, all on
// one stream, no side stream and none of the unchecked call's fusions:
//   shared, once    stages 0, 1, 2 of the checked key switch on the un-rotated c1                        (ksc_front)
//   per element     stage 3: inner product of the shared digits with the element's prepared key
//                   stage 8: sigma of the 2 M rows of the sums (into the plan's second set of sums) and of the L rows of c0
//                            (into the plan's rotation buffer), one sum check per row                    (galois_permute_checked)
//                   stages 4-7 on the rotated sums, sigma(c0) as the first part's addend                 (ksc_back)
// The unchecked call takes sigma on the loads of the special limbs' INTT and of the fused tail instead; both orders yield canonical
// residues of the same integers, so the words are fhe_rotate_hoisted's whichever route it took (fused, grouped, two streams).
#include "capi_checked.hpp"

HrcLayout hrc_layout(const fhe_keyswitch *p)
{
    const int L = p->L, K = p->K, M = L + K;
    const KscLayout k = ksc_layout(p, KsForm::CKKS);
    const int n[6] = {2 * M, 2 * M + L, 2 * K, 2 * (K + L), 2 * L, 2 * L};
    HrcLayout l{};
    for (int s = 0; s < 3; s++) l.shared[s] = k.off[s];
    l.n_shared = k.off[3];
    for (int i = 0; i < 6; i++) {
        l.rot[i] = l.n_rot;
        l.n_rot += n[i];
    }
    return l;
}

namespace {

// words of the flag buffer of n_rot rotations: the shared block, then one block per rotation
int hrc_flag_words(const HrcLayout &l, size_t n_rot, size_t *words)
{
    if (n_rot > (size_t)(0x7FFFFFFF - l.n_shared) / (size_t)l.n_rot) return fail(FHE_ERR_INVALID, "too many rotations for one flag buffer");
    *words = (size_t)l.n_shared + n_rot * l.n_rot;
    return FHE_OK;
}

} // namespace

int galois_fault_check(const GaloisFault &f, size_t units, int logn)
{
    if (f.point < 0) return FHE_OK;
    if (f.unit >= units || f.coeff >> logn) return fail(FHE_ERR_INVALID, "fault unit or coefficient outside the call");
    if (!galois_point_exists(f.point, f.bit, logn)) return fail(FHE_ERR_INVALID, "bad fault point: 0 takes a bit of the word, 1 a bit of the source index below log N");
    return FHE_OK;
}

int galois_permute_checked(fhe_ctx *ctx, hipStream_t st, const GalSeg *segs, int n_segs, int logn, u32 galois_elt, u32 *d_flags, const GaloisFault &f)
{
    size_t units = 0;
    for (int i = 0; i < n_segs; i++) units += segs[i].units;
    if (!units) return FHE_OK;
    // sigma_k^-1 = sigma_{k^-1 mod 2N}
    const u64 two_n = (u64)2 << logn;
    const u64 kinv = host::inv_mod(galois_elt % two_n, two_n);
    if (!kinv) return fail(FHE_ERR_INVALID, "Galois elements are odd");
    if (ctx->gal_sums.bytes < 2 * units * 8) HIP_TRY(ctx->gal_sums.alloc(2 * units * 8));
    u64 *s_in = ctx->gal_sums.as<u64>(), *s_out = s_in + units;
    HIP_TRY(hipMemsetAsync(s_in, 0, 2 * units * 8, st));
    size_t u0 = 0;
    for (int i = 0; i < n_segs; i++) {
        GaloisFault fi{};
        if (f.point >= 0 && f.unit >= u0 && f.unit < u0 + segs[i].units) {
            fi = f;
            fi.unit = (u32)(f.unit - u0);
        }
        hipError_t e = launch_automorphism_ntt_checked(st, segs[i].dst, segs[i].src, s_in + u0, s_out + u0, segs[i].units, logn, galois_elt, (u32)kinv, fi);
        if (e != hipSuccess) return hip_fail(e, "launch_automorphism_ntt_checked");
        u0 += segs[i].units;
    }
    hipError_t e = launch_galois_compare(st, d_flags, s_in, s_out, (u32)units);
    return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_galois_compare");
}

// the plan's buffers of the checked hoisted rotations and the test hook, checked against the call before anything is launched
int hrc_prepare(fhe_keyswitch *p, const StagedFault &ft, size_t n_rot, HrcHook &h)
{
    int rc;
    if ((rc = ksc_prepare(p))) return rc;
    // the rotated sums go into the plan's second set of sums (the unchecked hoisted rotations' side-stream set; allocated by whichever
    // call needs it first), sigma(c0) into the rotation buffer
    if (!p->acc2.p) HIP_TRY(p->acc2.alloc(p->acc.bytes));
    const int L = p->L, M = L + p->K;
    h = HrcHook{};
    if (ft.stage < 0) return FHE_OK;
    if (ft.stage >= 3 && (size_t)ft.block >= n_rot) return fail(FHE_ERR_INVALID, "fault rotation outside the call");
    h.rot = ft.block;
    if (ft.stage == 8) {
        h.gal = GaloisFault{ft.point, (u32)ft.unit, (u64)ft.coeff, ft.bit};
        if ((rc = galois_fault_check(h.gal, (size_t)2 * M + L, p->log_n))) return rc;
    } else if ((rc = ksc_hook(p, KsForm::CKKS, ft, p->acc2.as<u64>(), true, false, h.hook))) {
        return rc;
    }
    h.stage = ft.stage;
    return FHE_OK;
}

// the launches of the checked hoisted rotations; d_flags (the shared block, then one block per rotation) cleared by the caller
int hrc_run(fhe_keyswitch *p, uint64_t *const *d_out0, uint64_t *const *d_out1, const uint64_t *d_c0, const uint64_t *d_c1, const uint32_t *galois_elts,
            const uint64_t *const *d_prepared_keys, size_t n_rot, const fhe_abft *a, uint32_t *d_flags, hipStream_t st, const HrcHook &h,
            const HrcSealed *sealed)
{
    const HrcLayout lay = hrc_layout(p);
    u64 *acc_rot = p->acc2.as<u64>(), *c0_rot = p->rot.as<u64>();
    int rc;
    KscFlags fl{};
    for (int s = 0; s < 3; s++) fl.s[s] = d_flags + lay.shared[s];
    if ((rc = ksc_front(p, d_c1, a, fl, st, h.hook))) return rc;
    const KscHook none;
    static const int stage_of[6] = {3, 8, 4, 5, 6, 7};
    for (size_t r = 0; r < n_rot; r++) {
        u32 *block = d_flags + lay.n_shared + r * lay.n_rot;
        for (int i = 0; i < 6; i++) fl.s[stage_of[i]] = block + lay.rot[i];
        const bool armed = h.stage >= 3 && (size_t)h.rot == r;
        KscPerm perm{galois_elts[r], d_c0, acc_rot, c0_rot, armed ? h.gal : GaloisFault{}};
        if (!sealed) {
            if ((rc = ksc_back(p, d_out0[r], d_out1[r], d_c1, d_prepared_keys[r], nullptr, nullptr, a, fl, st, armed ? h.hook : none, &perm, KsForm::CKKS))) return rc;
            continue;
        }
        // the sealed call: the key verified on the inner product's load, c0 on the permutation's gather
        u32 *in = sealed->flags_in + r * sealed->stride;
        const SealedKeyStep key{sealed->seal_keys ? sealed->seal_keys[r] : nullptr, in + p->L, sealed->part, KsSealHit{0, 0, 0}};
        SealedSteps steps;
        steps.key = &key;
        if (sealed->seal_c0) {
            perm.seal_c0 = sealed->seal_c0;
            perm.flags_c0 = in;
            perm.part = sealed->part;
            if (sealed->hit.point >= 0 && sealed->hit_rot == r) perm.hit = sealed->hit;
        }
        if ((rc = ksc_back(p, d_out0[r], d_out1[r], d_c1, d_prepared_keys[r], nullptr, nullptr, a, fl, st, armed ? h.hook : none, &perm, KsForm::CKKS, steps)))
            return rc;
    }
    return FHE_OK;
}

extern "C" {

int fhe_automorphism_ntt_checked(fhe_ctx *ctx, uint64_t *d_dst, const uint64_t *d_src, int log_n, uint32_t galois_elt, size_t n_units,
                                 uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    const GaloisFault f = ctx->gal_fault.take();
    if (!d_dst || !d_src || !d_flags || d_dst == d_src || !(galois_elt & 1) || log_n < 1 || log_n > 30 || n_units > 0xFFFFFFFFull)
        return fail(FHE_ERR_INVALID, "bad automorphism arguments");
    int rc = galois_fault_check(f, n_units, log_n);
    if (rc) return rc;
    if (!n_units) return FHE_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const GalSeg seg{d_dst, d_src, (u32)n_units};
    return galois_permute_checked(ctx, pick(ctx, stream), &seg, 1, log_n, galois_elt, d_flags, f);
}

int fhe_ctx_inject_fault_galois(fhe_ctx *ctx, int point, int unit, long long coeff, int bit)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    return ctx->gal_fault.arm(GAL_AT_INDEX, point, unit, coeff, bit) ? FHE_OK : fail(FHE_ERR_INVALID, "bad fault");
}

int fhe_rotate_hoisted_checked_layout(const fhe_keyswitch *p, size_t n_rot, int out[12])
{
    if (!p || !out) return fail(FHE_ERR_INVALID, "null argument");
    const HrcLayout l = hrc_layout(p);
    size_t words;
    if (int rc = hrc_flag_words(l, n_rot, &words)) return rc;
    for (int s = 0; s < 3; s++) out[s] = l.shared[s];
    for (int i = 0; i < 6; i++) out[3 + i] = l.rot[i];
    out[9] = l.n_shared;
    out[10] = l.n_rot;
    out[11] = (int)words;
    return FHE_OK;
}

int fhe_ctx_inject_fault_rotate_hoisted(fhe_ctx *ctx, int rot, int stage, int point, int unit, long long coeff, int bit)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    return ctx->hrc_fault.arm(HRC_RULES, rot, stage, point, unit, coeff, bit) ? FHE_OK : fail(FHE_ERR_INVALID, "bad fault");
}

int fhe_rotate_hoisted_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *const *d_out0, uint64_t *const *d_out1, const uint64_t *d_c0,
                               const uint64_t *d_c1, const uint32_t *galois_elts, const uint64_t *const *d_prepared_keys, size_t n_rot,
                               const fhe_abft *a, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    const StagedFault ft = ctx->hrc_fault.take();
    int rc = ksc_scope(ctx, p, a, d_flags, KsForm::CKKS, false);
    if (rc) return rc;
    if (!d_c0 || !d_c1 || (n_rot && (!d_out0 || !d_out1 || !galois_elts || !d_prepared_keys))) return fail(FHE_ERR_INVALID, "null argument");
    for (size_t r = 0; r < n_rot; r++) {
        if (!d_out0[r] || !d_out1[r] || !d_prepared_keys[r]) return fail(FHE_ERR_INVALID, "null argument");
        if (!(galois_elts[r] & 1)) return fail(FHE_ERR_INVALID, "Galois elements are odd");
        if (d_out0[r] == d_c0 || d_out1[r] == d_c0 || d_out0[r] == d_c1 || d_out1[r] == d_c1 || d_out0[r] == d_out1[r])
            return fail(FHE_ERR_INVALID, "rotate is out of place");
    }
    if (!n_rot) return FHE_OK;
    size_t words;
    if ((rc = hrc_flag_words(hrc_layout(p), n_rot, &words))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    HrcHook hook;
    if ((rc = hrc_prepare(p, ft, n_rot, hook))) return rc;
    hipStream_t st = pick(ctx, stream);
    HIP_TRY(hipMemsetAsync(d_flags, 0, words * sizeof(u32), st));
    return hrc_run(p, d_out0, d_out1, d_c0, d_c1, galois_elts, d_prepared_keys, n_rot, a, d_flags, st, hook);
}

} // extern "C"
