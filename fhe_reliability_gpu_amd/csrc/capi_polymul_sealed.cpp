// capi_polymul_sealed.cpp -- the negacyclic product that verifies its factors' seals on the loads that transform them and writes its
// result's seal from the words it stores (polymul_seal.hpp, polymul_sealed.hip): fhe_polymul_sealed and its test hook (part of the C
// ABI of include/fhe_mi355x.h).
//
// The body of the sealed transforms (capi_ntt_fwd_sealed.cpp): the hooks are taken first -- its own and the checked product's --
// refusals come before anything is launched, the 5 * rows flag words are cleared, the launches run per run of an arithmetic path with
// seals, flags, partials and the hook's row addressed from the run's first limb, launch_compare_polymul closes block 2, and
// k_ntt_seal_out_finish writes each row's seal after all three blocks are final -- the poison rule: a row with any raised flag leaves
// the call with a seal that can never verify.  Seal partials live in the context's seal scratch ([a's][b's][c's]), the ABFT sums in
// the detector's psum as fhe_polymul_checked lays them out.  Whole-batch launches only.
#include "capi_sealed.hpp"

extern "C" {

int fhe_ctx_inject_fault_polymul_sealed(fhe_ctx *ctx, int operand, int row, long long coeff, int bit)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    return ctx->pm_seal_fault.arm(1, operand, 0, row, coeff, bit) ? FHE_OK : fail(FHE_ERR_INVALID, "bad fault");
}

int fhe_polymul_sealed(fhe_ctx *ctx, uint64_t *d_c, uint64_t *d_a, uint64_t *d_b, const fhe_ntt_tables *t, const fhe_abft *a, size_t n_poly, size_t limbs,
                       size_t start_idx, const uint64_t *d_seal_a, const uint64_t *d_seal_b, uint64_t *d_seal_c, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    const SealHook sf = ctx->pm_seal_fault.take();      // one shot each, whatever the outcome
    const PointFault pf = ctx->pm_fault.take();
    if (!d_a || !d_b || !d_c || !t || !a || !d_flags) return fail(FHE_ERR_INVALID, "null argument");
    if (a->t != t) return fail(FHE_ERR_INVALID, "the detector was made for another table set");
    int rc = check_range(t, n_poly, limbs, start_idx);
    if (rc) return rc;
    if (!t->has_inverse) return fail(FHE_ERR_UNSUPPORTED, "table set has no inverse (twiddle or N not invertible)");
    if (ctx->mode != 0 || ctx->resident || ctx->packed_on || ctx->only_pass >= 0 || !ntt_checked_supported(t->log_n) || !polymul_fused_supported(t->log_n))
        return fail(FHE_ERR_UNSUPPORTED, "the sealed product runs the checked fused product: not with ntt_mode=1, ntt_resident, ntt_packed, a single-pass hook, or N < 2^5");
    if (misaligned({d_a, d_b, d_c, d_seal_a, d_seal_b, d_seal_c})) return fail(FHE_ERR_INVALID, "sealed rows and seals must be 16-byte aligned");
    const bool square = d_a == d_b;
    if (square && d_seal_b && d_seal_b != d_seal_a) return fail(FHE_ERR_INVALID, "squaring: one factor has one seal (d_seal_b must be null or d_seal_a)");
    const size_t units = n_poly * limbs, N = (size_t)1 << t->log_n;
    SealedInputStep in[2] = {{d_seal_a, d_flags, nullptr, 0, 0, 0}, {square ? d_seal_a : d_seal_b, d_flags + units, nullptr, 0, 0, 0}};
    if (sf.sel >= 0) {
        if (sf.sel == 1 && square) return fail(FHE_ERR_INVALID, "squaring: there is no operand 1 to fault");
        if ((rc = ntt_seal_hit(sf, units, t->log_n, in[sf.sel]))) return rc;
    }
    // the checked product's hook, as fhe_polymul_checked takes it
    const int point = pf.point;
    const u64 fidx = pf.coeff;
    if (point >= 0) {
        if (point != 2 && t->log_n < 13)
            return fail(FHE_ERR_UNSUPPORTED, "fault point does not exist at this size / mode (0, 1, 3: two-launch sizes N >= 2^13; 2: the fused product)");
        if (fidx >= units * N) return fail(FHE_ERR_INVALID, "fault index outside the call's window");
    }
    if (!units) return FHE_OK;
    fhe_abft *m = const_cast<fhe_abft *>(a);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    PolymulSums s{};
    polymul_checked_tiles(t->log_n, &s.t_in, &s.t_mid, &s.t_out);
    if ((rc = polymul_sums(m, st, units, square, s))) return rc;
    // [a's input partials][b's][the product's output partials]: distinct regions, the single launch writes all three
    const size_t in_words = units * s.t_in * 3, out_words = d_seal_c ? units * s.t_out * 2 : 0;
    u64 *part;
    if ((rc = seal_scratch(ctx, st, 2 * in_words + out_words, &part))) return rc;
    in[0].part = part;
    in[1].part = part + in_words;
    u64 *part_c = d_seal_c ? part + 2 * in_words : nullptr;
    HIP_TRY(hipMemsetAsync(d_flags, 0, 5 * units * sizeof(u32), st));
    TraceScope tr(ctx, st, "POLYMUL_SEALED");
    const size_t hit_limb = ((size_t)fidx / N) % limbs;
    rc = for_each_run(t, limbs, start_idx, [&](size_t off, size_t len, int path) -> int {
        PassArgs pa{d_a + off * N, t->d_lp.as<LimbParams>(), (u32)(start_idx + off), (u32)len, (u32)(n_poly * len), (u32)limbs};
        PolymulChecks k{a->win.as<Tw>(), a->wout.as<Tw>(), a->wout8.as<u64>(), s, -1, nullptr, pf.bit};
        polymul_sums_from(k.s, off);
        if (point >= 0 && hit_limb >= off && hit_limb < off + len) {
            k.fault_point = point;
            k.fault_at = (point == 1 ? d_b : point == 3 ? d_c : d_a) + fidx;
        }
        const PolymulSealIo io{run_seal_in(in[0], off, len, limbs, s.t_in), run_seal_in(in[1], off, len, limbs, s.t_in), part_c ? part_c + off * s.t_out * 2 : nullptr};
        hipError_t e = launch_polymul_sealed(st, pa, d_b + off * N, d_c + off * N, t->log_n, path, k, io);
        return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_polymul_sealed");
    });
    if (rc) return rc;
    // squaring: one factor, one verdict -- block 1 repeats block 0
    if (square) HIP_TRY(hipMemcpyAsync(d_flags + units, d_flags, units * sizeof(u32), hipMemcpyDeviceToDevice, st));
    hipError_t e = launch_compare_polymul(st, d_flags + 2 * units, s, t->d_lp.as<LimbParams>(), (u32)start_idx, (u32)limbs, (u32)units);
    if (e != hipSuccess) return hip_fail(e, "launch_compare_polymul");
    if (!d_seal_c) return FHE_OK;
    e = launch_ntt_seal_out_finish(st, part_c, s.t_out, (u32)units, d_flags, d_flags + 2 * units, d_seal_c, d_flags + units, 3);
    return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_ntt_seal_out_finish");
}

} // extern "C"
