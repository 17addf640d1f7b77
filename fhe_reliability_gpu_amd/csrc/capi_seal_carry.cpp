// capi_seal_carry.cpp -- seals carried through the modular add and subtract (seal_carry.hpp, seal_carry.hip): fhe_modadd_sealed,
// fhe_modsub_sealed, their test hook, and the sealed rotate-and-sum (part of the C ABI of include/fhe_mi355x.h).
//
// The sealed multiply and rotation (capi_seal.cpp) verify, compute and seal in separate launches.  The add needs none of that: its
// one sweep holds the digest of the words it stores against the seal predicted from the operands' seals, on the load that feeds
// the adder, and writes the predicted seal.  fhe_rotate_sum_sealed is the tail of the reference's dot product
// (reliability_test/dotprod_test.cu:143-148) built from the two: per step fhe_rotate_sealed from the accumulators into the
// rotated copy, then one carried add per half back into the accumulators, seals updated in place.  A step's flag block is
//     [fhe_rotate_sealed_layout's block][add rows of c0: L][add rows of c1: L]
// and step s + 1 verifies on entry what step s's adds stored, so the chain needs no closing sweep.
#include "capi_sealed.hpp"
#include "seal_carry.hpp"

namespace {

// the carry hook as a call of n carry launches meets it: the record when it fires in one of them (*at = which), a disarmed one
// (*at = -1) when it is not armed or fires later -- those launches are then counted off
PointFault carry_take(fhe_ctx *ctx, int n, int *at)
{
    *at = -1;
    if (ctx->carry_fault.point < 0) return PointFault{};
    if (ctx->carry_skip >= n) {
        ctx->carry_skip -= n;
        return PointFault{};
    }
    *at = ctx->carry_skip;
    ctx->carry_skip = 0;
    return ctx->carry_fault.take();
}

PointwiseArgs carry_args(const fhe_ntt_tables *t, uint64_t *c, const uint64_t *a, const uint64_t *b, size_t n_poly, size_t limbs, size_t start_idx)
{
    return PointwiseArgs{c, a, b, t->d_lp.as<LimbParams>(), (u32)start_idx, (u32)limbs, (u32)(n_poly * limbs), (u32)limbs, t->log_n};
}

// fhe_modadd_sealed (sub == false) and fhe_modsub_sealed
int carry_body(bool sub, fhe_ctx *ctx, uint64_t *d_c, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_seal_c, const uint64_t *d_seal_a,
               const uint64_t *d_seal_b, uint64_t *d_locator_c, const uint64_t *d_locator_a, const uint64_t *d_locator_b, const fhe_ntt_tables *t,
               size_t n_poly, size_t limbs, size_t start_idx, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    int at;
    const PointFault f = carry_take(ctx, 1, &at);      // one shot, whatever the outcome
    if (!d_c || !d_a || !d_b || !d_flags) return fail(FHE_ERR_INVALID, "null argument");
    if (!d_seal_c || !d_seal_a || !d_seal_b) return fail(FHE_ERR_INVALID, "a carried add takes the seals of both operands and writes the result's: null seal");
    if (!d_locator_a != !d_locator_b || !d_locator_a != !d_locator_c) return fail(FHE_ERR_INVALID, "locators come in all three or none");
    int rc = check_range(t, n_poly, limbs, start_idx);
    if (rc) return rc;
    if (t->log_n < 1) return fail(FHE_ERR_UNSUPPORTED, "a sealed row has at least two words");
    if (misaligned({d_c, d_a, d_b})) return fail(FHE_ERR_INVALID, "sealed rows are read 16 bytes at a time: the buffers must be 16-byte aligned");
    const size_t units = n_poly * limbs;
    BcCheck k{d_flags, -1, 0, 0, 0};
    if ((rc = row_fault(f, f.point, units, t->log_n, k))) return rc;
    if (!units) return FHE_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    u64 *part;
    if ((rc = seal_scratch(ctx, st, carry_part_words((u32)units, t->log_n, d_locator_c != nullptr), &part))) return rc;
    HIP_TRY(hipMemsetAsync(d_flags, 0, units * sizeof(u32), st));
    hipError_t e = launch_modadd_carry(st, carry_args(t, d_c, d_a, d_b, n_poly, limbs, start_idx), sub, part, d_seal_a, d_seal_b, d_seal_c, d_locator_a,
                                       d_locator_b, d_locator_c, k);
    return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_modadd_carry");
}

} // namespace

extern "C" {

int fhe_ctx_inject_fault_seal_carry(fhe_ctx *ctx, int call, int point, int row, long long coeff, int bit)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    ctx->carry_skip = 0;
    if (row < 0) {
        (void)ctx->carry_fault.take();
        return FHE_OK;
    }
    if (call < 0 || point < 0 || !ctx->carry_fault.arm(CARRY_AT_WRAP, point, row, coeff, bit)) return fail(FHE_ERR_INVALID, "bad fault");
    ctx->carry_skip = call;
    return FHE_OK;
}

int fhe_modadd_sealed(fhe_ctx *ctx, uint64_t *d_c, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_seal_c, const uint64_t *d_seal_a,
                      const uint64_t *d_seal_b, uint64_t *d_locator_c, const uint64_t *d_locator_a, const uint64_t *d_locator_b, const fhe_ntt_tables *t,
                      size_t n_poly, size_t limbs, size_t start_idx, uint32_t *d_flags, void *stream)
{
    return carry_body(false, ctx, d_c, d_a, d_b, d_seal_c, d_seal_a, d_seal_b, d_locator_c, d_locator_a, d_locator_b, t, n_poly, limbs, start_idx, d_flags,
                      stream);
}

int fhe_modsub_sealed(fhe_ctx *ctx, uint64_t *d_c, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_seal_c, const uint64_t *d_seal_a,
                      const uint64_t *d_seal_b, uint64_t *d_locator_c, const uint64_t *d_locator_a, const uint64_t *d_locator_b, const fhe_ntt_tables *t,
                      size_t n_poly, size_t limbs, size_t start_idx, uint32_t *d_flags, void *stream)
{
    return carry_body(true, ctx, d_c, d_a, d_b, d_seal_c, d_seal_a, d_seal_b, d_locator_c, d_locator_a, d_locator_b, t, n_poly, limbs, start_idx, d_flags,
                      stream);
}

int fhe_rotate_sum_sealed_layout(const fhe_keyswitch *p, int n_steps, int out[4])
{
    if (!p || !out || n_steps < 1) return fail(FHE_ERR_INVALID, "bad argument");
    int lay[6];
    int rc = fhe_rotate_sealed_layout(p, lay);
    if (rc) return rc;
    out[0] = lay[4] + 2 * p->L;
    out[1] = lay[4];
    out[2] = n_steps * out[0];
    out[3] = 0;
    return FHE_OK;
}

int fhe_rotate_sum_sealed(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_c0, uint64_t *d_c1, uint64_t *d_tmp0, uint64_t *d_tmp1, int n_steps,
                          const uint32_t *galois_elts, const uint64_t *const *d_galois_keys, const fhe_abft *a, uint64_t *const *d_seal,
                          const uint64_t *const *d_seal_keys, uint64_t *const *d_seal_tmp, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    int at;
    const PointFault f = carry_take(ctx, n_steps > 0 ? 2 * n_steps : 0, &at);      // one shot, whatever the outcome
    if (n_steps < 1 || !galois_elts || !d_galois_keys) return fail(FHE_ERR_INVALID, "rotate-and-sum: at least one step, with its Galois element and key");
    if (!d_seal || !d_seal[0] || !d_seal[1] || !d_seal_tmp || !d_seal_tmp[0] || !d_seal_tmp[1])
        return fail(FHE_ERR_INVALID, "rotate-and-sum carries the seals of the accumulators and of the rotated copy: null seal");
    // what a later step would refuse is refused before the first one launches anything; everything else -- the scope of the checked
    // rotation included -- is step 0's to refuse, before its first launch
    bool bad = !d_c0 || !d_c1 || d_c0 == d_c1 || misaligned({d_c0, d_c1, d_tmp0, d_tmp1});
    for (int s = 0; s < n_steps; s++) bad = bad || !d_galois_keys[s] || !(galois_elts[s] & 1) || misaligned({d_galois_keys[s]});
    int lay[4], rc;
    if (bad || !p || fhe_rotate_sum_sealed_layout(p, n_steps, lay)) {
        rc = fhe_rotate_sealed(ctx, p, d_tmp0, d_tmp1, d_c0, d_c1, bad ? 0 : galois_elts[0], bad ? nullptr : d_galois_keys[0], a, nullptr, nullptr, nullptr,
                               d_flags, stream);      // refuses before its first launch, and takes the checked call's hook
        return rc ? rc : fail(FHE_ERR_INVALID, "rotate-and-sum: bad argument");
    }
    const size_t L = p->L;
    BcCheck armed{nullptr, -1, 0, 0, 0};
    if ((rc = row_fault(f, f.point, L, p->log_n, armed))) return rc;
    hipStream_t st = pick(ctx, stream);
    for (int s = 0; s < n_steps; s++) {
        uint32_t *block = d_flags + (size_t)s * lay[0];
        const uint64_t *seal_in[2] = {d_seal[0], d_seal[1]};
        rc = fhe_rotate_sealed(ctx, p, d_tmp0, d_tmp1, d_c0, d_c1, galois_elts[s], d_galois_keys[s], a, seal_in, d_seal_keys ? d_seal_keys[s] : nullptr,
                               d_seal_tmp, block, stream);
        if (rc) return rc;
        u64 *part;
        if ((rc = seal_scratch(ctx, st, carry_part_words((u32)L, p->log_n, false), &part))) return rc;
        HIP_TRY(hipMemsetAsync(block + lay[1], 0, 2 * L * sizeof(u32), st));
        uint64_t *acc[2] = {d_c0, d_c1};
        const uint64_t *rot[2] = {d_tmp0, d_tmp1};
        for (int h = 0; h < 2; h++) {
            BcCheck k = at == 2 * s + h ? armed : BcCheck{nullptr, -1, 0, 0, 0};
            k.flags = block + lay[1] + h * L;
            hipError_t e = launch_modadd_carry(st, carry_args(p->t, acc[h], acc[h], rot[h], 1, L, 0), false, part, d_seal[h], d_seal_tmp[h], d_seal[h], nullptr,
                                               nullptr, nullptr, k);
            if (e != hipSuccess) return hip_fail(e, "launch_modadd_carry");
        }
    }
    return FHE_OK;
}

} // extern "C"
