// capi_ntt_fwd_sealed.cpp -- the transforms that verify their input's seal on their own load and, where asked, write their
// output's seal from the words they store (ntt_seal_tap.hpp, ntt_sealed_io.hpp): fhe_ntt_inverse_sealed, fhe_ntt_forward_sealed,
// fhe_ntt_inverse_sealed_out and their test hook (part of the C ABI of include/fhe_mi355x.h), and what the sealed key switch
// (capi_ntt_sealed.cpp) shares with them: the hook's check against a call and the launch record of a run of limbs.
//
// One body for all three calls: the hooks are taken first, refusals come before anything is launched, the flag buffer is cleared,
// the launches run per run of an arithmetic path, and the ABFT comparison closes block 1.  With an output seal the output digest's
// partials live behind the input digest's in the context's seal scratch, and k_ntt_seal_out_finish writes each row's seal after
// both flag blocks are final -- the poison rule: a row with any raised flag leaves the call with a seal that can never verify.
#include "capi_sealed.hpp"

int ntt_seal_hit(const SealHook &f, size_t rows, int log_n, SealedInputStep &in)
{
    in.hit_row = in.hit_coeff = 0;
    in.hit_mask = 0;
    if (f.sel < 0) return FHE_OK;
    if (!f.inside(rows, log_n)) return fail(FHE_ERR_INVALID, "fault row or word outside the call");
    in.hit_row = (u32)f.row;
    in.hit_coeff = (u32)f.coeff;
    in.hit_mask = (u64)1 << f.bit;
    return FHE_OK;
}

// the sealed transform's record for the run of `len` limbs from limb `off` on, in a call whose row (poly, l) is row poly * limbs + l
// of the seal, the flags and the partials: all three and the hook's row are addressed from the run's first limb on
NttSealIn run_seal_in(const SealedInputStep &in, size_t off, size_t len, size_t limbs, u32 tin)
{
    NttSealIn s{in.seal ? in.seal + 2 * off : nullptr, in.flags + off, in.part + off * tin * 3};
    const size_t hl = in.hit_row % (limbs ? limbs : 1);
    if (in.hit_mask && hl >= off && hl < off + len) {
        s.hit_row = in.hit_row - (u32)off;
        s.hit_coeff = in.hit_coeff;
        s.hit_mask = in.hit_mask;
    }
    return s;
}

static int sealed_transform(bool inverse, fhe_ctx *ctx, uint64_t *d_dst, const uint64_t *d_src, const fhe_ntt_tables *t, const fhe_abft *a, size_t n_poly,
                            size_t limbs, size_t start_idx, const uint64_t *d_seal_src, uint64_t *d_seal_dst, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    const SealHook nf = ctx->ntt_seal_fault.take();      // one shot, whatever the outcome
    if (!d_dst || !d_src || !t || !a || !d_flags) return fail(FHE_ERR_INVALID, "null argument");
    if (a->t != t) return fail(FHE_ERR_INVALID, "the detector was made for another table set");
    int rc = check_range(t, n_poly, limbs, start_idx);
    if (rc) return rc;
    if (inverse && !t->has_inverse) return fail(FHE_ERR_UNSUPPORTED, "table set has no inverse (twiddle or N not invertible)");
    if (ctx->mode != 0 || ctx->resident || ctx->packed_on || ctx->only_pass >= 0 || !ntt_checked_supported(t->log_n))
        return fail(FHE_ERR_UNSUPPORTED, "the sealed transforms run the checked two-launch transform: not with ntt_mode=1, ntt_resident, ntt_packed, a single-pass hook, or N < 2^5");
    const size_t units = n_poly * limbs, N = (size_t)1 << t->log_n;
    SealedInputStep in{d_seal_src, d_flags, nullptr, 0, 0, 0};
    if ((rc = ntt_seal_hit(nf, units, t->log_n, in))) return rc;
    // the checked transforms' hook between the two launches (fhe_ctx_inject_fault), two-launch sizes, as the checked transforms take it
    const bool between = ctx->fault_idx >= 0 && t->log_n >= 13;
    const long long fidx = ctx->fault_idx;
    if (between) {
        ctx->fault_idx = -1;
        if ((u64)fidx >= units * N) return fail(FHE_ERR_INVALID, "fault index outside the call's window");
    }
    if (!units) return FHE_OK;
    fhe_abft *m = const_cast<fhe_abft *>(a);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    u32 tin = 1, tout = 1;
    ntt_checked_tiles(t->log_n, &tin, &tout, inverse);
    if (m->sum_in.bytes < units * 8 * tin || m->sum_out.bytes < units * 8 * tout) {
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(m->sum_in.alloc(units * 16 * tin));
        HIP_TRY(m->sum_out.alloc(units * 16 * tout));
    }
    // [the input digest's partials][the output digest's partials]: distinct regions, the single pass writes both in one launch
    const size_t in_words = ntt_seal_part_words((u32)units, t->log_n, inverse);
    const size_t out_words = d_seal_dst ? ntt_seal_out_part_words((u32)units, t->log_n, inverse) : 0;
    if ((rc = seal_scratch(ctx, st, in_words + out_words, &in.part))) return rc;
    u64 *part_out = d_seal_dst ? in.part + in_words : nullptr;
    HIP_TRY(hipMemsetAsync(d_flags, 0, 2 * units * sizeof(u32), st));
    // row (poly, l) of the call is row poly * limbs + l of the sums and of both digests; a run of limbs addresses them from its first limb on
    auto run = [&](int which) -> int {
        return for_each_run(t, limbs, start_idx, [&](size_t off, size_t len, int path) -> int {
            PassArgs pa{d_dst + off * N, t->d_lp.as<LimbParams>(), (u32)(start_idx + off), (u32)len, (u32)(n_poly * len), (u32)limbs, nullptr};
            if (d_src != d_dst) pa.src = d_src + off * N;
            const NttSealIn s = run_seal_in(in, off, len, limbs, tin);
            u64 *po = part_out ? part_out + off * tout * 2 : nullptr;
            u64 *si = m->sum_in.as<u64>() + off * tin, *so = m->sum_out.as<u64>() + off * tout;
            hipError_t e = launch_ntt_sealed(st, pa, a->win.as<Tw>(), a->wout.as<Tw>(), a->wout8.as<u64>(), si, so, t->log_n, path, which, inverse, s, po);
            return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_ntt_sealed");
        });
    };
    if (between) {
        if ((rc = run(0))) return rc;
        hipError_t e = launch_flip_bit(st, d_dst, (u64)fidx, ctx->fault_bit);
        if (e != hipSuccess) return hip_fail(e, "launch_flip_bit");
        if ((rc = run(1))) return rc;
    } else if ((rc = run(-1))) return rc;
    hipError_t e = launch_compare_sums(st, d_flags + units, m->sum_in.as<u64>(), tin, m->sum_out.as<u64>(), tout, t->d_lp.as<LimbParams>(), (u32)start_idx,
                                       (u32)limbs, (u32)units);
    if (e != hipSuccess) return hip_fail(e, "launch_compare_sums");
    if (!d_seal_dst) return FHE_OK;
    e = launch_ntt_seal_out_finish(st, part_out, tout, (u32)units, d_flags, d_flags + units, d_seal_dst);
    return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_ntt_seal_out_finish");
}

extern "C" {

int fhe_ctx_inject_fault_ntt_sealed(fhe_ctx *ctx, int row, long long coeff, int bit)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    return ctx->ntt_seal_fault.arm(INT_MAX, row, 0, row, coeff, bit) ? FHE_OK : fail(FHE_ERR_INVALID, "bad fault");
}

int fhe_ntt_inverse_sealed(fhe_ctx *ctx, uint64_t *d_dst, const uint64_t *d_src, const fhe_ntt_tables *t, const fhe_abft *a, size_t n_poly, size_t limbs,
                           size_t start_idx, const uint64_t *d_seal_src, uint32_t *d_flags, void *stream)
{
    return sealed_transform(true, ctx, d_dst, d_src, t, a, n_poly, limbs, start_idx, d_seal_src, nullptr, d_flags, stream);
}

int fhe_ntt_forward_sealed(fhe_ctx *ctx, uint64_t *d_dst, const uint64_t *d_src, const fhe_ntt_tables *t, const fhe_abft *a, size_t n_poly, size_t limbs,
                           size_t start_idx, const uint64_t *d_seal_src, uint64_t *d_seal_dst, uint32_t *d_flags, void *stream)
{
    return sealed_transform(false, ctx, d_dst, d_src, t, a, n_poly, limbs, start_idx, d_seal_src, d_seal_dst, d_flags, stream);
}

int fhe_ntt_inverse_sealed_out(fhe_ctx *ctx, uint64_t *d_dst, const uint64_t *d_src, const fhe_ntt_tables *t, const fhe_abft *a, size_t n_poly, size_t limbs,
                               size_t start_idx, const uint64_t *d_seal_src, uint64_t *d_seal_dst, uint32_t *d_flags, void *stream)
{
    return sealed_transform(true, ctx, d_dst, d_src, t, a, n_poly, limbs, start_idx, d_seal_src, d_seal_dst, d_flags, stream);
}

} // extern "C"
