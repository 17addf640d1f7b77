// capi_subscale_sealed.cpp -- the mod-down tail that verifies its input on load and seals its output on store (subscale_seal.hpp,
// subscale_sealed.hip): fhe_rescale_sealed, its layout and the test hook of the sealed tail (part of the C ABI of
// include/fhe_mi355x.h).  The tail as a step of a composite (SealedTailStep, capi_checked.hpp) is run by fhe_hmult_sealed_out
// (capi_seal.cpp) and fhe_rotate_sealed_out (capi_ntt_sealed.cpp).
//
// A caller with a sealed ciphertext could only compose fhe_seal_verify -> checked rescale -> fhe_seal: every input word was
// verified on one load and consumed on another (the last limbs on a third: sweep, copy into the plan, transform), and the outputs
// were sealed from a load after their store.  fhe_rescale_sealed is the checked rescale's launch list with two launches replaced:
// stage 0 is the sealed inverse transform (ntt_sealed.hip) out of place from the caller's last-limb rows into the plan -- no copy --
// and stage 3 is the sealed tail in its IN and OUT form.  Every load of the input is then a verified load, and the outputs' seals
// come from the stored registers.  The flag buffer is
//     [input rows, [n_parts][L]][the checked rescale's own block, exactly its layout]
// and a raised input flag does not stop the call: the words are the rescale of the input as it was loaded.
#include "capi_sealed.hpp"
#include "subscale_seal.hpp"

int subscale_seal_hit(const SealHook &f, size_t n_parts, size_t in_rows_per_part, size_t out_limbs, int log_n, SealedTailStep &tail)
{
    tail.hit_point = -1;
    if (f.sel < 0) return FHE_OK;
    if (f.sel == SS_AT_LOAD && !in_rows_per_part) return fail(FHE_ERR_INVALID, "fault point 0 (the load) needs an input seal step: this call runs the tail without one");
    if (f.sel == SS_AT_STORE && !out_limbs) return fail(FHE_ERR_INVALID, "fault point 1 (the store) needs output seals: this call was given none");
    const size_t per = f.sel == SS_AT_LOAD ? in_rows_per_part : out_limbs;
    if (!f.inside(n_parts * per, log_n)) return fail(FHE_ERR_INVALID, "fault row or word outside the call");
    if (f.sel == SS_AT_LOAD && (size_t)f.row % per == per - 1)
        return fail(FHE_ERR_INVALID, "fault row is a last-limb row: the tail does not load it (the sealed transform does, fhe_ctx_inject_fault_ntt_sealed)");
    tail.hit_point = f.sel;
    tail.hit_part = (u32)((size_t)f.row / per);
    tail.hit_limb = (u32)((size_t)f.row % per);
    tail.hit_coeff = (u32)f.coeff;
    tail.hit_mask = (u64)1 << f.bit;
    return FHE_OK;
}

extern "C" {

int fhe_ctx_inject_fault_subscale_sealed(fhe_ctx *ctx, int point, int row, long long coeff, int bit)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    return ctx->subscale_seal_fault.arm(SS_AT_STORE, point, 0, row, coeff, bit) ? FHE_OK : fail(FHE_ERR_INVALID, "bad fault");
}

int fhe_rescale_sealed_layout(const fhe_keyswitch *p, size_t n_parts, int out[4])
{
    if (!p || !out) return fail(FHE_ERR_INVALID, "null argument");
    if (n_parts < 1 || n_parts > 3) return fail(FHE_ERR_INVALID, "a ciphertext has 1 to 3 parts");
    if (p->L < 2) return fail(FHE_ERR_INVALID, "no prime left to drop");
    out[0] = 0;
    out[1] = (int)n_parts * p->L;
    out[2] = out[1] + rsc_layout(p, n_parts, sealed_form(p).form).total;
    out[3] = 0;
    return FHE_OK;
}

int fhe_rescale_sealed(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out, const uint64_t *d_in, size_t n_parts, const fhe_abft *a, const uint64_t *d_seal_in,
                       uint64_t *d_seal_out, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    const SealedForm f = sealed_form(p);
    // the three hooks belong to this call whatever its outcome
    const StagedFault ft = (ctx->*f.rs_hook).take();
    const SealHook nf = ctx->ntt_seal_fault.take();
    const SealHook tf = ctx->subscale_seal_fault.take();
    if (!d_seal_in) return fail(FHE_ERR_INVALID, "null d_seal_in: nothing would verify the input (fhe_rescale_checked takes none)");
    if (!d_seal_out) return fail(FHE_ERR_INVALID, "null d_seal_out: the outputs' seals have nowhere to go (fhe_rescale_checked writes none)");
    int rc = ksc_scope(ctx, p, a, d_flags, f.form, true);
    if (rc) return rc;
    if (!d_out || !d_in) return fail(FHE_ERR_INVALID, "null argument");
    if (n_parts < 1 || n_parts > 3) return fail(FHE_ERR_INVALID, "a ciphertext has 1 to 3 parts");
    if (p->log_n < 1) return fail(FHE_ERR_UNSUPPORTED, "a sealed row has at least two words");
    // input parts are L rows apart, output parts L - 1: any overlap of the output with the input is refused, as fhe_rescale does
    const size_t L = (size_t)p->L, R = L - 1, N = (size_t)1 << p->log_n, step = R * N;
    if (d_out < d_in + n_parts * L * N && d_in < d_out + n_parts * step) return fail(FHE_ERR_INVALID, "rescale is out of place");
    if (misaligned({d_out, d_in})) return fail(FHE_ERR_INVALID, "sealed rows are read 16 bytes at a time: the buffers must be 16-byte aligned");
    int lay[4];
    if ((rc = fhe_rescale_sealed_layout(p, n_parts, lay))) return rc;
    // every hook against the call, before anything is launched
    SealedTailStep tail{{d_seal_out, d_seal_out + 2 * R, d_seal_out + 4 * R}, nullptr};
    tail.seal_in = d_seal_in;
    tail.flags_in = d_flags + lay[0];
    if ((rc = subscale_seal_hit(tf, n_parts, L, R, p->log_n, tail))) return rc;
    if (nf.sel >= 0) {
        if (!nf.inside(n_parts * L, p->log_n)) return fail(FHE_ERR_INVALID, "fault row or word outside the call");
        if ((size_t)nf.row % L != R) return fail(FHE_ERR_INVALID, "fault row is not a last-limb row: the sealed transform loads those alone");
        tail.ntt_hit_part = (int)((size_t)nf.row / L);
        tail.ntt_hit_coeff = (u32)nf.coeff;
        tail.ntt_hit_mask = (u64)1 << nf.bit;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = ksc_prepare(p))) return rc;
    u64 *flip;
    if ((rc = rsc_hook(p, f.form, ft, n_parts, &flip))) return rc;      // (rescale_checked checks it again)
    hipStream_t st = pick(ctx, stream);
    const size_t tail_words = subscale_seal_part_words((u32)(2 * R), p->log_n, true);
    u64 *part;
    if ((rc = seal_scratch(ctx, st, tail_words + n_parts * ntt_seal_part_words(1, p->log_n, true), &part))) return rc;
    tail.part = part;
    tail.part_ntt = part + tail_words;
    HIP_TRY(hipMemsetAsync(d_flags, 0, (size_t)lay[1] * sizeof(u32), st));
    uint64_t *outs[3] = {d_out, d_out + step, d_out + 2 * step};
    return rescale_checked(p, f.form, outs, d_in, n_parts, a, d_flags + lay[1], st, ft, &tail);
}

} // extern "C"
