// capi_bsgs_checked.cpp -- the baby-step / giant-step matrix-vector product with every stage checked, and the checked modular add
// (part of the C ABI of include/fhe_mi355x.h; shared pieces in capi_checked.hpp).
//
// y = sum_{g < n2} sigma_{G_g}( sum_{b < n1} diag[g][b] * sigma_{B_b}(x) ), the product of fhe_bsgs_matvec (capi_keyswitch.cpp).  The
// launch list, all on one stream, no side stream and no fusion:
//   baby block (n1 > 1)   the checked hoisted rotations of x by the n1 - 1 baby elements into the plan's BSGS scratch   (hrc_run)
//   per giant step g      inner sum over the baby steps, both parts: into the outputs for g = 0, into scratch otherwise  (launch_diag_mac_checked)
//     g >= 1              sigma_{G_g} of the 2 L rows of the inner sum, rows of part 0 first                             (galois_permute_checked)
//                         t0 = out0 + sigma(s0)                                                                          (launch_modadd_checked)
//                         key switch of sigma(s1) with the giant key, addends (t0, out1), writing (out0, out1)           (keyswitch_checked)
// The running result rides on the addends of the key switch's tail, so a giant step needs ONE add launch: out1 has no term of its
// own besides the switch's second part, out0 has sigma(s0).  The tail (k_sub_scale_checked) reads add[i] and writes out[i] from the
// same lane and the two halves touch disjoint buffers, so d_out1 == d_add1 is in-place safe; t0 overwrites sigma(s0) in scratch
// (k_modadd_checked: c == b, same lane).  The unchecked call adds in another order (out + (tail + sigma(s0))) and takes sigma on
// loads; every stage yields canonical residues and those are unique, so the words are fhe_bsgs_matvec's bit for bit.
#include "capi_checked.hpp"
#include "bsgs_check.hpp"

#include <climits>

namespace {

struct BmcLayout {
    int baby, giant, off[4], total;      // words of the baby block, of one giant block; offsets of its four stages; total (-1: too large)
};

BmcLayout bmc_layout(const fhe_keyswitch *p, size_t n1, size_t n2)
{
    const int L = p->L;
    const HrcLayout h = hrc_layout(p);
    BmcLayout l{};
    const unsigned long long baby = n1 > 1 ? (unsigned long long)h.n_shared + (unsigned long long)(n1 - 1) * h.n_rot : 0;
    l.off[0] = 0;
    l.off[1] = 2 * L;
    l.off[2] = 4 * L;
    l.off[3] = 5 * L;
    l.giant = 5 * L + ksc_layout(p, KsForm::CKKS).total;
    const unsigned long long total = baby + (unsigned long long)n2 * l.giant;
    l.baby = (int)baby;
    l.total = total > (unsigned long long)INT_MAX ? -1 : (int)total;
    return l;
}

bool bsgs_shape_ok(size_t n1, size_t n2) { return n1 >= 1 && n2 >= 1 && n1 <= 4096 && n2 <= 4096; }

} // namespace

extern "C" {

int fhe_modadd_checked(fhe_ctx *ctx, uint64_t *c, const uint64_t *a, const uint64_t *b, const fhe_ntt_tables *t, size_t n_poly, size_t limbs,
                       size_t start_idx, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    // the one-shot pointwise hook belongs to this call whatever its outcome
    const PointFault f = ctx->pw_fault.take();
    if (!c || !a || !b || !d_flags) return fail(FHE_ERR_INVALID, "null argument");
    int rc = check_range(t, n_poly, limbs, start_idx);
    if (rc) return rc;
    const size_t units = n_poly * limbs;
    if (f.point >= 0 && !modadd_point_exists(f.point)) return fail(FHE_ERR_UNSUPPORTED, "fault points 0 (product) and 1 (quotient) do not exist on an add: 2 is the word, 3 the sum a + b");
    BcCheck k{d_flags, -1, 0, 0, 0};
    if ((rc = pointwise_fault(f, true, units << t->log_n, t->log_n, k))) return rc;
    if (!units) return FHE_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    HIP_TRY(hipMemsetAsync(d_flags, 0, units * sizeof(u32), st));
    const PointwiseArgs pa{c, a, b, t->d_lp.as<LimbParams>(), (u32)start_idx, (u32)limbs, (u32)units, (u32)limbs, t->log_n};
    hipError_t e = launch_modadd_checked(st, pa, k);
    return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_modadd_checked");
}

int fhe_bsgs_matvec_checked_layout(const fhe_keyswitch *p, size_t n1, size_t n2, int out[8])
{
    if (!p || !out) return fail(FHE_ERR_INVALID, "null argument");
    if (!bsgs_shape_ok(n1, n2)) return fail(FHE_ERR_INVALID, "n1 and n2 are 1 to 4096");
    const BmcLayout l = bmc_layout(p, n1, n2);
    if (l.total < 0) return fail(FHE_ERR_INVALID, "too many steps for one flag buffer");
    out[0] = 0;
    out[1] = l.baby;
    out[2] = l.giant;
    for (int s = 0; s < 4; s++) out[3 + s] = l.off[s];
    out[7] = l.total;
    return FHE_OK;
}

int fhe_ctx_inject_fault_bsgs(fhe_ctx *ctx, int g, int stage, int point, int unit, long long coeff, int bit)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    return ctx->bsgs_fault.arm(BSGS_RULES, g, stage, point, unit, coeff, bit) ? FHE_OK : fail(FHE_ERR_INVALID, "bad fault");
}

int fhe_bsgs_matvec_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1,
                            const uint64_t *d_diags, size_t n1, size_t n2, const uint32_t *baby_elts, const uint64_t *const *d_baby_keys_prepared,
                            const uint32_t *giant_elts, const uint64_t *const *d_giant_keys, const fhe_abft *a, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    // the one-shot hooks of the steps this call runs belong to it whatever its outcome: all are taken here
    const StagedFault hf = ctx->hrc_fault.take(), kf = ctx->ksc_fault.take(), bf = ctx->bsgs_fault.take();
    const GaloisFault gf = ctx->gal_fault.take();
    int rc = ksc_scope(ctx, p, a, d_flags, KsForm::CKKS, false);
    if (rc) return rc;
    if (!d_out0 || !d_out1 || !d_c0 || !d_c1 || !d_diags || !bsgs_shape_ok(n1, n2)) return fail(FHE_ERR_INVALID, "bad arguments");
    if ((n1 > 1 && (!baby_elts || !d_baby_keys_prepared)) || (n2 > 1 && (!giant_elts || !d_giant_keys))) return fail(FHE_ERR_INVALID, "null argument");
    for (size_t b = 0; b + 1 < n1; b++)
        if (!d_baby_keys_prepared[b] || !(baby_elts[b] & 1)) return fail(FHE_ERR_INVALID, "a baby step needs a prepared key and an odd Galois element");
    for (size_t g = 0; g + 1 < n2; g++)
        if (!d_giant_keys[g] || !(giant_elts[g] & 1)) return fail(FHE_ERR_INVALID, "a giant step needs a key and an odd Galois element");
    if (d_out0 == d_c0 || d_out0 == d_c1 || d_out1 == d_c0 || d_out1 == d_c1 || d_out0 == d_out1) return fail(FHE_ERR_INVALID, "the product is out of place");
    const BmcLayout lay = bmc_layout(p, n1, n2);
    if (lay.total < 0) return fail(FHE_ERR_INVALID, "too many steps for one flag buffer");
    HIP_TRY(hipSetDevice(ctx->device));
    const int L = p->L, logn = p->log_n;
    const size_t N = (size_t)1 << logn, part = (size_t)L * N;

    // ---- the test hooks, checked against this call before anything is launched
    HrcHook hh;
    if (n1 > 1) {
        if ((rc = hrc_prepare(p, hf, n1 - 1, hh))) return rc;
    } else {
        if ((rc = ksc_prepare(p))) return rc;
        if (hf.stage >= 0) return fail(FHE_ERR_INVALID, "hoisted-rotation fault outside the call: n1 = 1 has no baby block");
    }
    if ((kf.stage >= 0 || gf.point >= 0) && n2 < 2) return fail(FHE_ERR_INVALID, "key-switch or Galois fault outside the call: n2 = 1 has no giant rotation");
    if ((rc = galois_fault_check(gf, (size_t)2 * L, logn))) return rc;
    {
        KscHook probe;
        if ((rc = ksc_hook(p, KsForm::CKKS, kf, p->acc.as<u64>(), true, true, probe))) return rc;
    }
    if (bf.stage >= 0) {
        if ((size_t)bf.block >= n2 || (bf.stage == 1 && bf.block == 0)) return fail(FHE_ERR_INVALID, "fault giant step outside the call (the accumulate starts at g = 1)");
        if (bf.unit >= (bf.stage == 0 ? 2 * L : L) || (size_t)bf.coeff >= N) return fail(FHE_ERR_INVALID, "fault unit or coefficient outside the call");
        if (bf.stage == 1 && !modadd_point_exists(bf.point))
            return fail(FHE_ERR_UNSUPPORTED, "fault points 0 (product) and 1 (quotient) do not exist on the accumulate: 2 is the word, 3 the sum a + b");
    }

    hipStream_t st = pick(ctx, stream);
    // scratch: baby rotations [n1 - 1][2][L][N], inner sum [2][L][N], its permutation [2][L][N] (fhe_bsgs_matvec's own)
    const size_t need = ((n1 - 1) * 2 + 4) * part * 8;
    if (p->bsgs.bytes < need) {
        HIP_TRY(hipStreamSynchronize(st));        // (growing frees the old block)
        HIP_TRY(p->bsgs.alloc(need));
    }
    u64 *rot = p->bsgs.as<u64>(), *inner = rot + (n1 - 1) * 2 * part, *tmp = inner + 2 * part;
    HIP_TRY(hipMemsetAsync(d_flags, 0, (size_t)lay.total * sizeof(u32), st));

    // ---- baby block
    if (n1 > 1) {
        std::vector<u64 *> o0(n1 - 1), o1(n1 - 1);
        for (size_t b = 1; b < n1; b++) {
            o0[b - 1] = rot + (b - 1) * 2 * part;
            o1[b - 1] = o0[b - 1] + part;
        }
        if ((rc = hrc_run(p, o0.data(), o1.data(), d_c0, d_c1, baby_elts, d_baby_keys_prepared, n1 - 1, a, d_flags, st, hh))) return rc;
    }

    const LimbParams *lp = p->t->d_lp.as<LimbParams>();
    for (size_t g = 0; g < n2; g++) {
        u32 *block = d_flags + lay.baby + g * lay.giant;
        // ---- inner sum of giant step g: straight into the result for g = 0
        u64 *s0 = g ? inner : d_out0, *s1 = g ? inner + part : d_out1;
        const DiagMacArgs da{s0, s1, d_diags + g * n1 * part, d_c0, d_c1, rot, lp, 0u, (u32)L, (u32)n1, logn};
        hipError_t e = launch_diag_mac_checked(st, da, bc_check(bf.at((int)g, 0), block + lay.off[0]));
        if (e != hipSuccess) return hip_fail(e, "launch_diag_mac_checked");
        if (!g) continue;
        // ---- sigma of both parts of the inner sum
        const GalSeg seg{tmp, inner, (u32)(2 * L)};
        if ((rc = galois_permute_checked(ctx, st, &seg, 1, logn, giant_elts[g - 1], block + lay.off[1], g == 1 ? gf : GaloisFault{}))) return rc;
        // ---- t0 = out0 + sigma(s0), in place over sigma(s0)
        const PointwiseArgs pa{tmp, d_out0, tmp, lp, 0u, (u32)L, (u32)L, (u32)L, logn};
        if ((e = launch_modadd_checked(st, pa, bc_check(bf.at((int)g, 1), block + lay.off[2]))) != hipSuccess) return hip_fail(e, "launch_modadd_checked");
        // ---- (out0, out1) = key switch of sigma(s1) + (t0, out1)
        if ((rc = keyswitch_checked(p, KsForm::CKKS, d_out0, d_out1, tmp + part, d_giant_keys[g - 1], tmp, d_out1, a, block + lay.off[3], st, g == 1 ? kf : StagedFault{}))) return rc;
    }
    return FHE_OK;
}

} // extern "C"
