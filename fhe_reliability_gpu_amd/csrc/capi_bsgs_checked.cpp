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
//
// fhe_bsgs_matvec_sealed is the same body in another mode (SealedMode, the RepairMode pattern of capi_seal.cpp): it verifies the
// given seals of c0, c1 and of every baby (as prepared) and giant key with sweeps of their own, runs the baby block unchanged, runs
// per giant step the inner sum that digests each diagonal word from the register it multiplies (launch_diag_mac_sealed; n1 > 16: a
// verifying sweep over the step's diagonal rows, then launch_diag_mac_checked) and seals both outputs.  Its flag buffer is
//     [c0 L][c1 L][baby keys (n1 - 1) key_rows][giant keys (n2 - 1) key_rows][diagonals n2 n1 L][the checked call's own block]
#include "capi_sealed.hpp"
#include "bsgs_seal.hpp"

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

// the mode of the body that is fhe_bsgs_matvec_sealed: the seals that come with the operands (HOST arrays of device pointers; an
// array or an entry may be null: that operand is not verified) and where the outputs' seals go -- a null SealedMode is the checked call
struct SealedMode {
    const uint64_t *const *seal_in;          // [2]: c0, c1, [L][2] each
    const uint64_t *const *seal_baby;        // [n1 - 1]: the prepared baby keys, [key_rows][2] each
    const uint64_t *const *seal_giant;       // [n2 - 1]: the giant keys
    const uint64_t *seal_diag;               // [n2][n1][L][2]
    uint64_t *const *seal_out;               // [2]
};

// offsets of c0, c1, the baby keys, the giant keys, the diagonals and the checked block; total (-1: too large)
struct BmsLayout {
    int off[6], total;
};

BmsLayout bms_layout(const fhe_keyswitch *p, size_t n1, size_t n2)
{
    const unsigned long long L = p->L, kr = key_rows(p);
    const BmcLayout c = bmc_layout(p, n1, n2);
    unsigned long long o[7];
    o[0] = 0;
    o[1] = L;
    o[2] = 2 * L;
    o[3] = o[2] + (n1 - 1) * kr;
    o[4] = o[3] + (n2 - 1) * kr;
    o[5] = o[4] + (unsigned long long)n2 * n1 * L;
    o[6] = o[5] + (c.total < 0 ? 0 : c.total);
    BmsLayout l{};
    for (int i = 0; i < 6; i++) l.off[i] = o[i] > (unsigned long long)INT_MAX ? INT_MAX : (int)o[i];
    l.total = c.total < 0 || o[6] > (unsigned long long)INT_MAX ? -1 : (int)o[6];
    return l;
}

// fhe_bsgs_matvec_checked (sm == nullptr) and fhe_bsgs_matvec_sealed
int bsgs_body(const SealedMode *sm, fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1,
              const uint64_t *d_diags, size_t n1, size_t n2, const uint32_t *baby_elts, const uint64_t *const *d_baby_keys_prepared,
              const uint32_t *giant_elts, const uint64_t *const *d_giant_keys, const fhe_abft *a, uint32_t *d_flags, void *stream);

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
    return bsgs_body(nullptr, ctx, p, d_out0, d_out1, d_c0, d_c1, d_diags, n1, n2, baby_elts, d_baby_keys_prepared, giant_elts, d_giant_keys, a, d_flags, stream);
}

int fhe_bsgs_matvec_sealed_layout(const fhe_keyswitch *p, size_t n1, size_t n2, int out[8])
{
    if (!p || !out) return fail(FHE_ERR_INVALID, "null argument");
    if (!bsgs_shape_ok(n1, n2)) return fail(FHE_ERR_INVALID, "n1 and n2 are 1 to 4096");
    const BmsLayout l = bms_layout(p, n1, n2);
    if (l.total < 0) return fail(FHE_ERR_INVALID, "too many steps for one flag buffer");
    for (int i = 0; i < 6; i++) out[i] = l.off[i];
    out[6] = l.total;
    out[7] = 0;
    return FHE_OK;
}

int fhe_ctx_inject_fault_bsgs_sealed(fhe_ctx *ctx, int g, int b, int limb, long long coeff, int bit)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    return ctx->bsgs_seal_fault.arm(INT_MAX, g, b, limb, coeff, bit) ? FHE_OK : fail(FHE_ERR_INVALID, "bad fault");
}

int fhe_bsgs_matvec_sealed(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1,
                           const uint64_t *d_diags, size_t n1, size_t n2, const uint32_t *baby_elts, const uint64_t *const *d_baby_keys_prepared,
                           const uint32_t *giant_elts, const uint64_t *const *d_giant_keys, const fhe_abft *a, const uint64_t *const *d_seal_in,
                           const uint64_t *const *d_seal_baby_keys, const uint64_t *const *d_seal_giant_keys, const uint64_t *d_seal_diags,
                           uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream)
{
    const SealedMode sm{d_seal_in, d_seal_baby_keys, d_seal_giant_keys, d_seal_diags, d_seal_out};
    return bsgs_body(&sm, ctx, p, d_out0, d_out1, d_c0, d_c1, d_diags, n1, n2, baby_elts, d_baby_keys_prepared, giant_elts, d_giant_keys, a, d_flags, stream);
}

} // extern "C"

namespace {

int bsgs_body(const SealedMode *sm, fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1,
              const uint64_t *d_diags, size_t n1, size_t n2, const uint32_t *baby_elts, const uint64_t *const *d_baby_keys_prepared,
              const uint32_t *giant_elts, const uint64_t *const *d_giant_keys, const fhe_abft *a, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    // the one-shot hooks of the steps this call runs belong to it whatever its outcome: all are taken here
    const StagedFault hf = ctx->hrc_fault.take(), kf = ctx->ksc_fault.take(), bf = ctx->bsgs_fault.take();
    const GaloisFault gf = ctx->gal_fault.take();
    const SealHook sf = sm ? ctx->bsgs_seal_fault.take() : SealHook{};
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
    const int L = p->L, logn = p->log_n;
    const size_t N = (size_t)1 << logn, part = (size_t)L * N;
    BmsLayout sl{};
    if (sm) {
        sl = bms_layout(p, n1, n2);
        if (sl.total < 0) return fail(FHE_ERR_INVALID, "too many steps for one flag buffer");
        bool bad = misaligned({d_out0, d_out1, d_c0, d_c1, d_diags});
        for (size_t b = 0; b + 1 < n1; b++) bad = bad || misaligned({d_baby_keys_prepared[b]});
        for (size_t g = 0; g + 1 < n2; g++) bad = bad || misaligned({d_giant_keys[g]});
        if (bad) return fail(FHE_ERR_INVALID, "sealed rows are read 16 bytes at a time: the buffers must be 16-byte aligned");
        if (sf.sel >= 0) {
            if ((size_t)sf.sel >= n2 || (size_t)sf.idx >= n1 || !sf.inside((size_t)L, logn))
                return fail(FHE_ERR_INVALID, "sealed-diagonal fault outside the call");
            if (!sm->seal_diag) return fail(FHE_ERR_INVALID, "sealed-diagonal fault outside the call: no diagonal seals were given");
        }
    }
    HIP_TRY(hipSetDevice(ctx->device));

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
    const bool fused = sm && sm->seal_diag && n1 <= DIAG_SEAL_MAX_NB;
    u64 *spart = nullptr;
    u32 *d_sealed = d_flags;      // the sealed call's buffer; d_flags becomes the checked call's own block inside it
    if (sm) {
        // the partial-sum scratch of the context, sized once for the largest sweep of the call, before the first launch
        size_t words = std::max(seal_part_words((u32)key_rows(p), logn), seal_part_words((u32)L, logn));
        if (sm->seal_diag) words = std::max(words, fused ? diag_seal_part_words((u32)L, logn, diag_seal_nb((u32)n1)) : seal_part_words((u32)(n1 * L), logn));
        if ((rc = seal_scratch(ctx, st, words, &spart))) return rc;
        HIP_TRY(hipMemsetAsync(d_sealed, 0, (size_t)sl.off[5] * sizeof(u32), st));
        d_flags = d_sealed + sl.off[5];
        // ---- the operands and keys at rest: a raised flag does not stop the call
        const uint64_t *ops[2] = {d_c0, d_c1};
        for (int h = 0; h < 2; h++)
            if ((rc = verify_rows(st, seal_args(p->t, ops[h], 1, L, 0), sm->seal_in ? sm->seal_in[h] : nullptr, d_sealed + sl.off[h], spart))) return rc;
        const size_t kr = key_rows(p);
        for (size_t b = 0; b + 1 < n1; b++)
            if ((rc = verify_rows(st, seal_args(p->t, d_baby_keys_prepared[b], (size_t)p->dnum * 2, L + p->K, 0), sm->seal_baby ? sm->seal_baby[b] : nullptr,
                                  d_sealed + sl.off[2] + b * kr, spart)))
                return rc;
        for (size_t g = 0; g + 1 < n2; g++)
            if ((rc = verify_rows(st, seal_args(p->t, d_giant_keys[g], (size_t)p->dnum * 2, L + p->K, 0), sm->seal_giant ? sm->seal_giant[g] : nullptr,
                                  d_sealed + sl.off[3] + g * kr, spart)))
                return rc;
    }
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
        hipError_t e;
        if (sm && sm->seal_diag) {
            // ---- the diagonal rows of this step against their seals: on the load that feeds the product, or (n1 > 16) in a sweep before it
            u32 *dflags = d_sealed + sl.off[4] + g * n1 * L;
            const u64 *dseal = sm->seal_diag + g * n1 * L * 2;
            const bool hit = sf.sel == (int)g;
            if (fused) {
                const DiagHit dh{(u32)sf.idx, (u32)sf.row, (u64)sf.coeff, hit ? (u64)1 << sf.bit : 0};
                if ((e = launch_diag_mac_sealed(st, da, spart, dseal, dflags, bc_check(bf.at((int)g, 0), block + lay.off[0]), dh)) != hipSuccess)
                    return hip_fail(e, "launch_diag_mac_sealed");
            } else {
                const BcCheck hook{nullptr, hit ? 0 : -1, (u32)(sf.idx * L + sf.row), (u64)sf.coeff, (u64)1 << sf.bit};
                if ((rc = verify_rows(st, seal_args(p->t, da.diag, n1, L, 0), dseal, dflags, spart, &hook))) return rc;
            }
        }
        if (!fused && (e = launch_diag_mac_checked(st, da, bc_check(bf.at((int)g, 0), block + lay.off[0]))) != hipSuccess)
            return hip_fail(e, "launch_diag_mac_checked");
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
    // ---- both outputs sealed for the next sealed call
    return sm ? seal_outputs(st, p->t, sm->seal_out, nullptr, d_out0, d_out1, L, spart) : FHE_OK;
}

} // namespace
