// capi_galois_sealed.cpp -- the Galois permutation that verifies its source's seal on its own gather (galois_seal.hpp,
// galois_sealed.hip): fhe_automorphism_ntt_sealed, the sealed hoisted rotations with their layout, and the one-shot test hook (part
// of the C ABI of include/fhe_mi355x.h).
//
// fhe_rotate_hoisted_sealed is fhe_rotate_hoisted_checked's launch list (hrc_run) with three additions.  The flag buffer is
//     [c1 rows L][per rotation r: [c0 rows L][key rows dnum 2 M]][fhe_rotate_hoisted_checked's block, exactly its layout]
//   c1              verified once, by a sweep: its consuming load is inside the transform kernels of stage 0 (the shared INTT), which
//                   no digest can ride on, so verifying load and consuming load stay two loads
//   per rotation    stage 3 runs through a SealedKeyStep with the prepared key's seal: the key is verified on the load that
//                   multiplies it (above KS_SEAL_MAX_DNUM digits: the sweep followed by k_ks_mac_checked, as elsewhere);
//                   stage 8 sends the 2 M rows of the sums through the checked permutation as before and, when c0's seal is given,
//                   the L rows of c0 through k_automorphism_ntt_sealed<false, .>: every rotation verifies c0 on its own gather and
//                   no sweep over c0 exists.  Their verdict lands in that rotation's [c0 rows]; their L words of the stage-8 block
//                   stay zero.  Without c0's seal c0 goes through the checked permutation exactly as in the checked call
//   outputs         both sealed, one sweep each
// A raised input flag does not stop the call.  CKKS form only, like the checked call.
#include "capi_sealed.hpp"
#include "galois_seal.hpp"

namespace {

// the hook as a call took it, checked against that call: n_rot rotations (1 for the standalone call) of `rows` rows
int gal_seal_hit(const SealHook &f, size_t n_rot, size_t rows, int log_n, GalSealHit &hit)
{
    hit = GalSealHit{-1, 0, 0, 0};
    if (f.sel < 0) return FHE_OK;
    if ((size_t)f.idx >= n_rot || !f.inside(rows, log_n)) return fail(FHE_ERR_INVALID, "fault rotation, row or word outside the call");
    if (!galois_point_exists(f.sel, f.bit, log_n)) return fail(FHE_ERR_INVALID, "bad fault point: 0 takes a bit of the word, 1 a bit of the source index below log N");
    hit = GalSealHit{f.sel, (u32)f.row, (u32)f.coeff, (u64)1 << f.bit};
    return FHE_OK;
}

} // namespace

extern "C" {

int fhe_ctx_inject_fault_galois_sealed(fhe_ctx *ctx, int rot, int point, int row, long long coeff, int bit)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    return ctx->gal_seal_fault.arm(GAL_AT_INDEX, point, rot, row, coeff, bit) ? FHE_OK : fail(FHE_ERR_INVALID, "bad fault");
}

int fhe_automorphism_ntt_sealed(fhe_ctx *ctx, uint64_t *d_dst, const uint64_t *d_src, uint64_t *d_seal_dst, const uint64_t *d_seal_src,
                                const fhe_ntt_tables *t, size_t n_poly, size_t limbs, size_t start_idx, uint32_t galois_elt, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    const SealHook gf = ctx->gal_seal_fault.take();      // one shot, whatever the outcome
    if (!d_dst || !d_src || !d_flags) return fail(FHE_ERR_INVALID, "null argument");
    if (!d_seal_src) return fail(FHE_ERR_INVALID, "a sealed permutation takes the source's seal: null seal (without one nothing checks the permutation)");
    if (d_dst == d_src) return fail(FHE_ERR_INVALID, "the permutation is out of place");
    if (!(galois_elt & 1)) return fail(FHE_ERR_INVALID, "Galois elements are odd");
    int rc = check_range(t, n_poly, limbs, start_idx);
    if (rc) return rc;
    if (t->log_n < 1) return fail(FHE_ERR_UNSUPPORTED, "a sealed row has at least two words");
    if (misaligned({d_dst, d_src})) return fail(FHE_ERR_INVALID, "sealed rows are stored 16 bytes at a time: the buffers must be 16-byte aligned");
    const size_t units = n_poly * limbs;
    if (units > 0xFFFFFFFFull) return fail(FHE_ERR_INVALID, "too many rows");
    GalSealHit hit;
    if ((rc = gal_seal_hit(gf, 1, units, t->log_n, hit))) return rc;
    if (!units) return FHE_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    u64 *part;
    if ((rc = seal_scratch(ctx, st, galois_seal_part_words((u32)units, t->log_n, d_seal_dst != nullptr), &part))) return rc;
    HIP_TRY(hipMemsetAsync(d_flags, 0, units * sizeof(u32), st));
    const GalSealArgs ga{d_dst, d_src, t->d_lp.as<LimbParams>(), (u32)start_idx, (u32)limbs, (u32)units, (u32)limbs, t->log_n, galois_elt};
    hipError_t e = launch_automorphism_ntt_sealed(st, ga, part, d_seal_src, d_seal_dst, d_flags, hit);
    return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_automorphism_ntt_sealed");
}

int fhe_rotate_hoisted_sealed_layout(const fhe_keyswitch *p, size_t n_rot, int out[6])
{
    if (!p || !out) return fail(FHE_ERR_INVALID, "null argument");
    if (p->plain_modulus) return fail(FHE_ERR_UNSUPPORTED, "the sealed hoisted rotations run the CKKS form: not on a plan with a plain modulus");
    int inner[12];
    int rc = fhe_rotate_hoisted_checked_layout(p, n_rot, inner);
    if (rc) return rc;
    const size_t L = (size_t)p->L, per = L + key_rows(p);
    if (n_rot > ((size_t)0x7FFFFFFF - L - (size_t)inner[11]) / per) return fail(FHE_ERR_INVALID, "too many rotations for one flag buffer");
    out[0] = 0;                                 // c1 rows
    out[1] = (int)L;                            // rotation 0's input block: [c0 rows L][key rows dnum 2 M]
    out[2] = (int)per;                          // words per rotation input block
    out[3] = (int)(L + n_rot * per);            // the checked call's block
    out[4] = out[3] + inner[11];                // total
    out[5] = ks_sealed_fused(p) ? 1 : 0;
    return FHE_OK;
}

int fhe_rotate_hoisted_sealed(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *const *d_out0, uint64_t *const *d_out1, const uint64_t *d_c0, const uint64_t *d_c1,
                              const uint32_t *galois_elts, const uint64_t *const *d_prepared_keys, size_t n_rot, const fhe_abft *a,
                              const uint64_t *const *d_seal_in, const uint64_t *const *d_seal_keys, uint64_t *const *d_seal_out0,
                              uint64_t *const *d_seal_out1, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    // both hooks belong to this call whatever its outcome
    const StagedFault ft = ctx->hrc_fault.take();
    const SealHook gf = ctx->gal_seal_fault.take();
    int rc = ksc_scope(ctx, p, a, d_flags, KsForm::CKKS, false);
    if (rc) return rc;
    if (!d_c0 || !d_c1 || (n_rot && (!d_out0 || !d_out1 || !galois_elts || !d_prepared_keys))) return fail(FHE_ERR_INVALID, "null argument");
    if (misaligned({d_c0, d_c1})) return fail(FHE_ERR_INVALID, "sealed rows are read 16 bytes at a time: the buffers must be 16-byte aligned");
    for (size_t r = 0; r < n_rot; r++) {
        if (!d_out0[r] || !d_out1[r] || !d_prepared_keys[r]) return fail(FHE_ERR_INVALID, "null argument");
        if (!(galois_elts[r] & 1)) return fail(FHE_ERR_INVALID, "Galois elements are odd");
        if (d_out0[r] == d_c0 || d_out1[r] == d_c0 || d_out0[r] == d_c1 || d_out1[r] == d_c1 || d_out0[r] == d_out1[r])
            return fail(FHE_ERR_INVALID, "rotate is out of place");
        if (misaligned({d_out0[r], d_out1[r], d_prepared_keys[r]}))
            return fail(FHE_ERR_INVALID, "sealed rows are read 16 bytes at a time: the buffers must be 16-byte aligned");
    }
    const uint64_t *seal_c0 = d_seal_in ? d_seal_in[0] : nullptr, *seal_c1 = d_seal_in ? d_seal_in[1] : nullptr;
    const int L = p->L, M = L + p->K;
    HrcSealed sealed{seal_c0, d_seal_keys, nullptr, 0, nullptr, GalSealHit{-1, 0, 0, 0}, 0};
    if (gf.sel >= 0 && !seal_c0) return fail(FHE_ERR_INVALID, "fault outside the call: without c0's seal no sealed permutation runs");
    if ((rc = gal_seal_hit(gf, n_rot, (size_t)L, p->log_n, sealed.hit))) return rc;
    sealed.hit_rot = gf.sel >= 0 ? (size_t)gf.idx : 0;
    if (!n_rot) return FHE_OK;
    int lay[6];
    if ((rc = fhe_rotate_hoisted_sealed_layout(p, n_rot, lay))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    HrcHook hook;
    if ((rc = hrc_prepare(p, ft, n_rot, hook))) return rc;
    // a stage-8 fault on a c0 row has no launch to hit when c0 goes through the sealed permutation
    if (seal_c0 && hook.stage == 8 && hook.gal.unit >= (u32)(2 * M))
        return fail(FHE_ERR_INVALID, "fault outside the call: with c0's seal the checked permutation covers the sums only");
    hipStream_t st = pick(ctx, stream);
    const size_t words = std::max({ks_sealed_scratch_words(p), seal_part_words((u32)L, p->log_n), galois_seal_part_words((u32)L, p->log_n, false)});
    if ((rc = seal_scratch(ctx, st, words, &sealed.part))) return rc;
    sealed.flags_in = d_flags + lay[1];
    sealed.stride = (size_t)lay[2];
    HIP_TRY(hipMemsetAsync(d_flags, 0, (size_t)lay[4] * sizeof(u32), st));
    if ((rc = verify_rows(st, seal_args(p->t, d_c1, 1, L, 0), seal_c1, d_flags + lay[0], sealed.part))) return rc;
    if ((rc = hrc_run(p, d_out0, d_out1, d_c0, d_c1, galois_elts, d_prepared_keys, n_rot, a, d_flags + lay[3], st, hook, &sealed))) return rc;
    for (size_t r = 0; r < n_rot; r++) {
        uint64_t *const seals[2] = {d_seal_out0 ? d_seal_out0[r] : nullptr, d_seal_out1 ? d_seal_out1[r] : nullptr};
        if ((rc = seal_outputs(st, p->t, seals, nullptr, d_out0[r], d_out1[r], L, sealed.part))) return rc;
    }
    return FHE_OK;
}

} // extern "C"
