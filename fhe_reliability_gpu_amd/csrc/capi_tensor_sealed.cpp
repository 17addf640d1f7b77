// capi_tensor_sealed.cpp -- the tensor product with its operands verified on the load that multiplies them (tensor_seal.hpp,
// tensor_sealed.hip): fhe_tensor_product_sealed, its layout and its test hook (part of the C ABI of include/fhe_mi355x.h), and the
// launches behind them as the sealed tensor step of a composite (fhe_hmult_sealed_fused, capi_seal.cpp).
//
// fhe_hmult_sealed verifies a0, a1, b0, b1 in four sweeps and multiplies from a second load.  Here one launch loads every operand
// word once, digests it from the register that is handed to the product, and digests d0, d1, d2 from the registers it stores; a
// finish launch holds the operands' sums against the stored seals and writes the results' seals.  The flag buffer is
//     [rows of a0][rows of a1][rows of b0][rows of b1][the tensor block, [rows][3] as fhe_tensor_product_checked's]
// with R = n_poly * limbs rows each.  A raised operand flag does not stop the call: the words are the product of the operands as
// they were loaded, and the residue identity holds on them.
#include "capi_sealed.hpp"
#include "tensor_seal.hpp"

int tensor_seal_hit(const SealHook &f, size_t units, int log_n, TensorSealHit &hit)
{
    hit = TensorSealHit{-1, 0, 0, 0};
    if (f.sel < 0) return FHE_OK;
    if (!f.inside(units, log_n)) return fail(FHE_ERR_INVALID, "fault row or word outside the call");
    hit = TensorSealHit{f.sel, (u32)f.row, (u64)f.coeff, (u64)1 << f.bit};
    return FHE_OK;
}

size_t tensor_sealed_scratch_words(size_t units, int log_n, bool out) { return tensor_seal_part_words((u32)units, log_n, out); }

int tensor_sealed_run(fhe_ctx *ctx, hipStream_t st, uint64_t *const d[3], const uint64_t *const ops[4], const fhe_ntt_tables *t, size_t n_poly, size_t limbs,
                      size_t start_idx, const uint64_t *const *seal_in, uint64_t *const *seal_out, uint32_t *const flags_op[4], const BcCheck &k,
                      const TensorSealHit &hit)
{
    TensorSealArgs ta{d[0], d[1], d[2], ops[0], ops[1], ops[2], ops[3], t->d_lp.as<LimbParams>(), (u32)start_idx, (u32)limbs, (u32)(n_poly * limbs), t->log_n,
                      {}, {}, {}};
    for (int o = 0; o < 4; o++) {
        ta.seal_in[o] = seal_in ? seal_in[o] : nullptr;
        ta.flags_op[o] = flags_op[o];
    }
    bool out = false;
    for (int i = 0; i < 3; i++) {
        ta.seal_out[i] = seal_out ? seal_out[i] : nullptr;
        out = out || ta.seal_out[i];
    }
    u64 *part;
    const int rc = seal_scratch(ctx, st, tensor_seal_part_words(ta.units, t->log_n, out), &part);
    if (rc) return rc;
    hipError_t e = launch_tensor_sealed(st, ta, part, k, hit);
    return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_tensor_sealed");
}

extern "C" {

int fhe_ctx_inject_fault_tensor_sealed(fhe_ctx *ctx, int operand, int row, long long coeff, int bit)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    return ctx->tensor_seal_fault.arm(3, operand, 0, row, coeff, bit) ? FHE_OK : fail(FHE_ERR_INVALID, "bad fault");
}

int fhe_tensor_product_sealed_layout(size_t n_poly, size_t limbs, int out[6])
{
    if (!out) return fail(FHE_ERR_INVALID, "null argument");
    if (n_poly * limbs > ((size_t)1 << 24)) return fail(FHE_ERR_INVALID, "batch too large for one launch (max 2^24 limb-polynomials)");
    const int R = (int)(n_poly * limbs);
    for (int i = 0; i < 5; i++) out[i] = i * R;
    out[5] = 7 * R;
    return FHE_OK;
}

int fhe_tensor_product_sealed(fhe_ctx *ctx, uint64_t *d_d0, uint64_t *d_d1, uint64_t *d_d2, const uint64_t *d_a0, const uint64_t *d_a1, const uint64_t *d_b0,
                              const uint64_t *d_b1, const fhe_ntt_tables *t, size_t n_poly, size_t limbs, size_t start_idx, const uint64_t *const *d_seal_in,
                              uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    // both hooks belong to this call whatever its outcome
    const PointFault pf = ctx->pw_fault.take();
    const SealHook tf = ctx->tensor_seal_fault.take();
    if (!d_d0 || !d_d1 || !d_d2 || !d_a0 || !d_a1 || !d_b0 || !d_b1 || !d_flags) return fail(FHE_ERR_INVALID, "null argument");
    int rc = check_range(t, n_poly, limbs, start_idx);
    if (rc) return rc;
    if (t->log_n < 1) return fail(FHE_ERR_UNSUPPORTED, "a sealed row has at least two words");
    if (misaligned({d_d0, d_d1, d_d2, d_a0, d_a1, d_b0, d_b1})) return fail(FHE_ERR_INVALID, "sealed rows are read 16 bytes at a time: the buffers must be 16-byte aligned");
    const size_t R = n_poly * limbs;
    int lay[6];
    if ((rc = fhe_tensor_product_sealed_layout(n_poly, limbs, lay))) return rc;
    BcCheck k{d_flags + lay[4], -1, 0, 0, 0};
    if ((rc = pointwise_fault(pf, true, R << t->log_n, t->log_n, k))) return rc;
    TensorSealHit hit;
    if ((rc = tensor_seal_hit(tf, R, t->log_n, hit))) return rc;
    if (!R) return FHE_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    HIP_TRY(hipMemsetAsync(d_flags, 0, (size_t)lay[5] * sizeof(u32), st));
    uint64_t *const d[3] = {d_d0, d_d1, d_d2};
    const uint64_t *const ops[4] = {d_a0, d_a1, d_b0, d_b1};
    uint32_t *const flags_op[4] = {d_flags + lay[0], d_flags + lay[1], d_flags + lay[2], d_flags + lay[3]};
    return tensor_sealed_run(ctx, st, d, ops, t, n_poly, limbs, start_idx, d_seal_in, d_seal_out, flags_op, k, hit);
}

} // extern "C"
