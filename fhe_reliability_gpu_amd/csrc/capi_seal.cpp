// capi_seal.cpp -- seals of operands at rest (seal_check.hpp, seal_checked.hip): fhe_seal, fhe_seal_verify, their test hook, and the
// sealed homomorphic multiply and rotation (part of the C ABI of include/fhe_mi355x.h).
//
// The checked calls do not cover faults already in their inputs.  A sealed composite closes that gap around an existing checked
// call without touching it: it verifies every seal it was given (operands, key), runs the checked call's own body (hmult_checked,
// rotate_checked of capi_checked.hpp) -- in the CKKS or the BGV form and with that form's hooks, by the plan's plain modulus -- and
// seals both outputs, all on one stream.  The flag buffer is
//     [input rows, in argument order][key rows][the checked call's own block, exactly its layout]
// and a raised input flag does not stop the call: flags are read by the caller afterwards, as everywhere else.
//
// Repair (seal_repair.hip): fhe_seal_locator writes the third sum of a row, fhe_seal_repair is fhe_seal_verify's sweep followed by
// k_row_repair, and the repairing composites are the sealed composites' own bodies in another mode (RepairMode): each given
// (seal, locator) pair is repaired in place instead of only verified, the outputs get locators when asked, and one report block
// follows the flags, covering the input and key rows in the order of their flag words.
#include "capi_sealed.hpp"

namespace {

int seal_window(const fhe_ntt_tables *t, const uint64_t *d_words, size_t n_poly, size_t limbs, size_t start_idx)
{
    int rc = check_range(t, n_poly, limbs, start_idx);
    if (rc) return rc;
    if (t->log_n < 1) return fail(FHE_ERR_UNSUPPORTED, "a sealed row has at least two words");
    if ((uintptr_t)d_words % 16) return fail(FHE_ERR_INVALID, "sealed rows are read 16 bytes at a time: the buffer must be 16-byte aligned");
    return FHE_OK;
}

// the mode of a sealed composite that repairs its operands and key instead of only verifying them: the locators that go with the
// seals (HOST arrays as the seals'; entries may be null) -- a null RepairMode is the verifying call
struct RepairMode {
    const uint64_t *const *loc_in;
    const uint64_t *loc_key;
    uint64_t *const *loc_out;
};

// one operand of a sealed composite: `limbs` rows from table limb 0 on, n_poly polynomials; a null seal is skipped, a locator
// makes the rows repaired in place (the words are then written)
struct SealedRows {
    const uint64_t *words, *seal, *locator;
    size_t n_poly, limbs;
    int flag_off;
};

// the operand verified and, with a locator, repaired; d_report = the report block of the whole call, one record of four words per
// flag word of the input and key rows
int verify_or_repair(hipStream_t st, const fhe_ntt_tables *t, const SealedRows &r, uint32_t *d_flags, uint64_t *d_report, u64 *part)
{
    const SealArgs sa = seal_args(t, r.words, r.n_poly, r.limbs, 0);
    const int rc = verify_rows(st, sa, r.seal, d_flags + r.flag_off, part);
    if (rc || !r.seal || !r.locator) return rc;
    hipError_t e = launch_seal_repair(st, sa, r.seal, r.locator, d_flags + r.flag_off, d_report + 4 * (size_t)r.flag_off);
    return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_seal_repair");
}

// a repairing call takes seal and locator of an operand together or not at all
bool unpaired(const RepairMode *rm, const uint64_t *const *d_seal_in, int n, const uint64_t *d_seal_key)
{
    if (!rm) return false;
    for (int i = 0; i < n; i++)
        if (!(d_seal_in && d_seal_in[i]) != !(rm->loc_in && rm->loc_in[i])) return true;
    return !d_seal_key != !rm->loc_key;
}

// where the report block of a repairing composite starts, in flag words: 16-byte aligned after the sealed call's layout
int report_offset(int sealed_total) { return (sealed_total + 3) & ~3; }

// scratch for the largest launch of a sealed composite (the key's rows; tensor: or the sealed tensor step's), before anything is
// launched
int sealed_scratch(fhe_ctx *ctx, hipStream_t st, const fhe_keyswitch *p, bool tensor, u64 **part)
{
    // (the sealed tail's partials, [2 L][chunks][2], are never more than the key's)
    const size_t key = seal_part_words((u32)key_rows(p), p->log_n);
    return seal_scratch(ctx, st, tensor ? std::max(key, tensor_sealed_scratch_words((size_t)p->L, p->log_n, false)) : key, part);
}

} // namespace

extern "C" {

int fhe_ctx_inject_fault_seal(fhe_ctx *ctx, int row, long long coeff, int bit)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    return ctx->seal_fault.arm(0, row < 0 ? -1 : 0, row, coeff, bit) ? FHE_OK : fail(FHE_ERR_INVALID, "bad fault");
}

int fhe_seal(fhe_ctx *ctx, uint64_t *d_seal, const uint64_t *d_words, const fhe_ntt_tables *t, size_t n_poly, size_t limbs, size_t start_idx,
             void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    const PointFault f = ctx->seal_fault.take();      // one shot, whatever the outcome
    if (!d_seal || !d_words) return fail(FHE_ERR_INVALID, "null argument");
    int rc = seal_window(t, d_words, n_poly, limbs, start_idx);
    if (rc) return rc;
    const size_t units = n_poly * limbs;
    BcCheck k{nullptr, -1, 0, 0, 0};
    if ((rc = row_fault(f, 0, units, t->log_n, k))) return rc;
    if (!units) return FHE_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    u64 *part;
    if ((rc = seal_scratch(ctx, st, seal_part_words((u32)units, t->log_n), &part))) return rc;
    hipError_t e = launch_seal(st, seal_args(t, d_words, n_poly, limbs, start_idx), part, d_seal, k);
    return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_seal");
}

int fhe_seal_verify(fhe_ctx *ctx, const uint64_t *d_words, const uint64_t *d_seal, const fhe_ntt_tables *t, size_t n_poly, size_t limbs,
                    size_t start_idx, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    const PointFault f = ctx->seal_fault.take();      // one shot, whatever the outcome
    if (!d_seal || !d_words || !d_flags) return fail(FHE_ERR_INVALID, "null argument");
    int rc = seal_window(t, d_words, n_poly, limbs, start_idx);
    if (rc) return rc;
    const size_t units = n_poly * limbs;
    BcCheck k{d_flags, -1, 0, 0, 0};
    if ((rc = row_fault(f, 0, units, t->log_n, k))) return rc;
    if (!units) return FHE_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    u64 *part;
    if ((rc = seal_scratch(ctx, st, seal_part_words((u32)units, t->log_n), &part))) return rc;
    HIP_TRY(hipMemsetAsync(d_flags, 0, units * sizeof(u32), st));
    hipError_t e = launch_seal_verify(st, seal_args(t, d_words, n_poly, limbs, start_idx), part, d_seal, k);
    return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_seal_verify");
}

int fhe_seal_locator(fhe_ctx *ctx, uint64_t *d_locator, const uint64_t *d_words, const fhe_ntt_tables *t, size_t n_poly, size_t limbs, size_t start_idx,
                     void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    if (!d_locator || !d_words) return fail(FHE_ERR_INVALID, "null argument");
    int rc = seal_window(t, d_words, n_poly, limbs, start_idx);
    if (rc) return rc;
    const size_t units = n_poly * limbs;
    if (!units) return FHE_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    u64 *part;
    if ((rc = seal_scratch(ctx, st, seal_part_words((u32)units, t->log_n), &part))) return rc;
    hipError_t e = launch_seal_locator(st, seal_args(t, d_words, n_poly, limbs, start_idx), part, d_locator);
    return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_seal_locator");
}

int fhe_seal_repair(fhe_ctx *ctx, uint64_t *d_words, const uint64_t *d_seal, const uint64_t *d_locator, const fhe_ntt_tables *t, size_t n_poly,
                    size_t limbs, size_t start_idx, uint32_t *d_flags, uint64_t *d_report, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    const PointFault f = ctx->seal_fault.take();      // one shot, whatever the outcome
    if (!d_seal || !d_words || !d_flags || !d_locator || !d_report) return fail(FHE_ERR_INVALID, "null argument");
    int rc = seal_window(t, d_words, n_poly, limbs, start_idx);
    if (rc) return rc;
    if ((uintptr_t)d_report % 16) return fail(FHE_ERR_INVALID, "a report record is written 16 bytes at a time: the buffer must be 16-byte aligned");
    const size_t units = n_poly * limbs;
    BcCheck k{d_flags, -1, 0, 0, 0};
    if ((rc = row_fault(f, 0, units, t->log_n, k))) return rc;
    if (!units) return FHE_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    u64 *part;
    if ((rc = seal_scratch(ctx, st, seal_part_words((u32)units, t->log_n), &part))) return rc;
    HIP_TRY(hipMemsetAsync(d_flags, 0, units * sizeof(u32), st));
    const SealArgs sa = seal_args(t, d_words, n_poly, limbs, start_idx);
    hipError_t e = launch_seal_verify(st, sa, part, d_seal, k);      // the hook lives in this sweep only
    if (e != hipSuccess) return hip_fail(e, "launch_seal_verify");
    e = launch_seal_repair(st, sa, d_seal, d_locator, d_flags, d_report);
    return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_seal_repair");
}

int fhe_hmult_sealed_layout(const fhe_keyswitch *p, int rescale, int out[8])
{
    if (!p || !out) return fail(FHE_ERR_INVALID, "null argument");
    int inner[4];
    int rc = hmult_checked_layout(p, sealed_form(p).form, rescale, inner);
    if (rc) return rc;
    for (int i = 0; i < 4; i++) out[i] = i * p->L;
    out[4] = 4 * p->L;
    out[5] = out[4] + (int)key_rows(p);
    out[6] = out[5] + inner[3];
    out[7] = 0;
    return FHE_OK;
}

// fhe_hmult_sealed (rm == nullptr), fhe_hmult_sealed_repair and fhe_hmult_sealed_fused (fused, never with rm: repair needs the
// sweep).  fused: the four operand sweeps are gone and the checked multiply's tensor step is the sealed tensor product
// (capi_tensor_sealed.cpp), which verifies a0, a1, b0, b1 on the load that multiplies them and writes their row flags where the
// sweeps wrote them; the key's sweep, the key switch, the rescale and the output seals are the same launches.  fused_key
// (fhe_hmult_sealed_fused_key, with fused): the key's sweep is gone as well and the key switch's inner product is the sealed one
// (capi_keyswitch_sealed.cpp), which verifies the key on the load that multiplies it and writes the key rows' flags where the
// sweep wrote them; the call takes that step's hook.  out (fhe_hmult_sealed_out, with fused_key): the two output sweeps are gone as
// well and the multiply's last launch is the sealed tail (capi_subscale_sealed.cpp), which writes the outputs' seals from the
// registers it stores; the call takes that step's hook
static int hmult_sealed_body(const RepairMode *rm, bool fused, bool fused_key, bool out, fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_a0,
                             const uint64_t *d_a1, const uint64_t *d_b0, const uint64_t *d_b1, const uint64_t *d_relin_key, int rescale, const fhe_abft *a,
                             const uint64_t *const *d_seal_in, const uint64_t *d_seal_key, uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    const SealedForm f = sealed_form(p);
    SealedTensorStep step{d_seal_in, {nullptr, nullptr, nullptr, nullptr}};
    SealedKeyStep kstep{d_seal_key, nullptr, nullptr, KsSealHit{0, 0, 0}};
    SealedTailStep tstep{{d_seal_out ? d_seal_out[0] : nullptr, d_seal_out ? d_seal_out[1] : nullptr, nullptr}, nullptr};
    const SealHook kf = fused_key ? ctx->ks_seal_fault.take() : SealHook{};      // one shot, whatever the outcome
    const SealHook tf = out ? ctx->subscale_seal_fault.take() : SealHook{};
    auto checked = [&](uint32_t *flags) {
        return hmult_checked(f.form, f.ks_hook, f.rs_hook, ctx, p, d_out0, d_out1, d_a0, d_a1, d_b0, d_b1, d_relin_key, rescale, a, flags, stream,
                             fused ? &step : nullptr, fused_key ? &kstep : nullptr, out ? &tstep : nullptr);
    };
    // what must hold before the first verifying launch, so that a call outside the checked call's scope launches nothing: the
    // checked call itself then refuses (it returns the status and takes its hooks)
    if (ksc_scope(ctx, p, a, d_flags, f.form, rescale != 0) || !d_out0 || !d_out1 || d_out0 == d_out1 || !d_a0 || !d_a1 || !d_b0 || !d_b1 || !d_relin_key) {
        const int rc = checked(d_flags);      // refuses before its first launch
        return rc ? rc : fail(FHE_ERR_INVALID, "sealed multiply: bad argument");
    }
    if (misaligned({d_out0, d_out1, d_a0, d_a1, d_b0, d_b1, d_relin_key, rm ? d_flags : nullptr})) {
        (void)checked(nullptr);      // takes the hooks, launches nothing
        return fail(FHE_ERR_INVALID, "sealed rows are read 16 bytes at a time: the buffers must be 16-byte aligned");
    }
    if (unpaired(rm, d_seal_in, 4, d_seal_key)) {
        (void)checked(nullptr);
        return fail(FHE_ERR_INVALID, "a repairing call takes an operand's seal and locator together");
    }
    int lay[8], rc;
    if ((rc = fhe_hmult_sealed_layout(p, rescale, lay))) return rc;
    if (fused) {
        // the sealed tensor product's hook is checked against the call before the key's sweep is launched
        TensorSealHit hit;
        if (tensor_seal_hit(ctx->tensor_seal_fault, (size_t)p->L, p->log_n, hit)) {
            (void)checked(nullptr);      // takes the hooks, launches nothing
            return fail(FHE_ERR_INVALID, "fault row or word outside the call");
        }
        for (int i = 0; i < 4; i++) step.flags_op[i] = d_flags + lay[i];
    }
    if (fused_key && ks_seal_hit(kf, p, kstep.hit)) {
        (void)checked(nullptr);      // takes the hooks, launches nothing
        return fail(FHE_ERR_INVALID, "fault key row or word outside the call");
    }
    const size_t out_limbs = tstep.seal_out[0] && tstep.seal_out[1] ? (size_t)(rescale ? p->L - 1 : p->L) : 0;
    if (out && subscale_seal_hit(tf, 2, 0, out_limbs, p->log_n, tstep)) {
        (void)checked(nullptr);      // takes the hooks, launches nothing
        return subscale_seal_hit(tf, 2, 0, out_limbs, p->log_n, tstep);      // the status and its message
    }
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    u64 *part;
    if ((rc = sealed_scratch(ctx, st, p, fused, &part))) return rc;
    kstep.flags_key = d_flags + lay[4];
    kstep.part = tstep.part = part;      // the key's verdict is out before the tail starts on the same stream
    HIP_TRY(hipMemsetAsync(d_flags, 0, (size_t)lay[5] * sizeof(u32), st));
    uint64_t *d_report = rm ? reinterpret_cast<uint64_t *>(d_flags + report_offset(lay[6])) : nullptr;
    if (rm) HIP_TRY(hipMemsetAsync(d_report, 0, (size_t)lay[5] * 4 * sizeof(u64), st));      // rows without a seal report CLEAN
    const size_t L = p->L;
    const uint64_t *ops[4] = {d_a0, d_a1, d_b0, d_b1};
    for (int i = 0; i < 4 && !fused; i++) {
        const SealedRows r{ops[i], d_seal_in ? d_seal_in[i] : nullptr, rm && rm->loc_in ? rm->loc_in[i] : nullptr, 1, L, lay[i]};
        if ((rc = verify_or_repair(st, p->t, r, d_flags, d_report, part))) return rc;
    }
    const SealedRows key{d_relin_key, d_seal_key, rm ? rm->loc_key : nullptr, (size_t)p->dnum * 2, L + p->K, lay[4]};
    if (!fused_key && (rc = verify_or_repair(st, p->t, key, d_flags, d_report, part))) return rc;
    if ((rc = checked(d_flags + lay[5])) || out) return rc;
    return seal_outputs(st, p->t, d_seal_out, rm ? rm->loc_out : nullptr, d_out0, d_out1, rescale ? L - 1 : L, part);
}

int fhe_hmult_sealed_out(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_a0, const uint64_t *d_a1,
                         const uint64_t *d_b0, const uint64_t *d_b1, const uint64_t *d_relin_key, int rescale, const fhe_abft *a,
                         const uint64_t *const *d_seal_in, const uint64_t *d_seal_key, uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream)
{
    return hmult_sealed_body(nullptr, true, true, true, ctx, p, d_out0, d_out1, d_a0, d_a1, d_b0, d_b1, d_relin_key, rescale, a, d_seal_in, d_seal_key, d_seal_out,
                             d_flags, stream);
}

int fhe_hmult_sealed_fused(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_a0, const uint64_t *d_a1,
                           const uint64_t *d_b0, const uint64_t *d_b1, const uint64_t *d_relin_key, int rescale, const fhe_abft *a,
                           const uint64_t *const *d_seal_in, const uint64_t *d_seal_key, uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream)
{
    return hmult_sealed_body(nullptr, true, false, false, ctx, p, d_out0, d_out1, d_a0, d_a1, d_b0, d_b1, d_relin_key, rescale, a, d_seal_in, d_seal_key, d_seal_out,
                             d_flags, stream);
}

int fhe_hmult_sealed_fused_key(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_a0, const uint64_t *d_a1,
                               const uint64_t *d_b0, const uint64_t *d_b1, const uint64_t *d_relin_key, int rescale, const fhe_abft *a,
                               const uint64_t *const *d_seal_in, const uint64_t *d_seal_key, uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream)
{
    return hmult_sealed_body(nullptr, true, true, false, ctx, p, d_out0, d_out1, d_a0, d_a1, d_b0, d_b1, d_relin_key, rescale, a, d_seal_in, d_seal_key, d_seal_out,
                             d_flags, stream);
}

int fhe_hmult_sealed(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_a0, const uint64_t *d_a1,
                     const uint64_t *d_b0, const uint64_t *d_b1, const uint64_t *d_relin_key, int rescale, const fhe_abft *a,
                     const uint64_t *const *d_seal_in, const uint64_t *d_seal_key, uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream)
{
    return hmult_sealed_body(nullptr, false, false, false, ctx, p, d_out0, d_out1, d_a0, d_a1, d_b0, d_b1, d_relin_key, rescale, a, d_seal_in, d_seal_key, d_seal_out, d_flags,
                             stream);
}

int fhe_hmult_sealed_repair_layout(const fhe_keyswitch *p, int rescale, int out[10])
{
    int rc = fhe_hmult_sealed_layout(p, rescale, out);
    if (rc) return rc;
    out[7] = report_offset(out[6]);
    out[8] = out[7] + 8 * out[5];
    out[9] = 0;
    return FHE_OK;
}

int fhe_hmult_sealed_repair(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, uint64_t *d_a0, uint64_t *d_a1, uint64_t *d_b0,
                            uint64_t *d_b1, uint64_t *d_relin_key, int rescale, const fhe_abft *a, const uint64_t *const *d_seal_in,
                            const uint64_t *const *d_locator_in, const uint64_t *d_seal_key, const uint64_t *d_locator_key,
                            uint64_t *const *d_seal_out, uint64_t *const *d_locator_out, uint32_t *d_flags, void *stream)
{
    const RepairMode rm{d_locator_in, d_locator_key, d_locator_out};
    return hmult_sealed_body(&rm, false, false, false, ctx, p, d_out0, d_out1, d_a0, d_a1, d_b0, d_b1, d_relin_key, rescale, a, d_seal_in, d_seal_key, d_seal_out, d_flags,
                             stream);
}

int fhe_rotate_sealed_layout(const fhe_keyswitch *p, int out[6])
{
    if (!p || !out) return fail(FHE_ERR_INVALID, "null argument");
    out[0] = 0;
    out[1] = p->L;
    out[2] = 2 * p->L;
    out[3] = out[2] + (int)key_rows(p);
    out[4] = out[3] + ksc_layout(p, sealed_form(p).form).total;
    out[5] = 0;
    return FHE_OK;
}

// fhe_rotate_sealed (rm == nullptr), fhe_rotate_sealed_repair and fhe_rotate_sealed_fused (fused_key, never with rm: repair needs
// the sweep).  fused_key: the sweeps over c0 and c1 stay, the key's sweep is gone and the key switch's inner product is the sealed
// one (capi_keyswitch_sealed.cpp), which writes the key rows' flags where the sweep wrote them; the call takes that step's hook
static int rotate_sealed_body(const RepairMode *rm, bool fused_key, fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0,
                              const uint64_t *d_c1, uint32_t galois_elt, const uint64_t *d_galois_key, const fhe_abft *a, const uint64_t *const *d_seal_in,
                              const uint64_t *d_seal_key, uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    const SealedForm f = sealed_form(p);
    SealedKeyStep kstep{d_seal_key, nullptr, nullptr, KsSealHit{0, 0, 0}};
    const SealHook kf = fused_key ? ctx->ks_seal_fault.take() : SealHook{};      // one shot, whatever the outcome
    auto checked = [&](uint32_t *flags) {
        return rotate_checked(f.form, f.ks_hook, ctx, p, d_out0, d_out1, d_c0, d_c1, galois_elt, d_galois_key, a, flags, stream, fused_key ? &kstep : nullptr);
    };
    if (ksc_scope(ctx, p, a, d_flags, f.form, false) || !d_out0 || !d_out1 || d_out0 == d_out1 || !d_c0 || !d_c1 || !d_galois_key || !(galois_elt & 1)) {
        const int rc = checked(d_flags);      // refuses before its first launch
        return rc ? rc : fail(FHE_ERR_INVALID, "sealed rotation: bad argument");
    }
    if (misaligned({d_out0, d_out1, d_c0, d_c1, d_galois_key, rm ? d_flags : nullptr})) {
        (void)checked(nullptr);      // takes the hook, launches nothing
        return fail(FHE_ERR_INVALID, "sealed rows are read 16 bytes at a time: the buffers must be 16-byte aligned");
    }
    if (unpaired(rm, d_seal_in, 2, d_seal_key)) {
        (void)checked(nullptr);
        return fail(FHE_ERR_INVALID, "a repairing call takes an operand's seal and locator together");
    }
    int lay[6], rc;
    if ((rc = fhe_rotate_sealed_layout(p, lay))) return rc;
    if (fused_key && ks_seal_hit(kf, p, kstep.hit)) {
        (void)checked(nullptr);      // takes the hook, launches nothing
        return fail(FHE_ERR_INVALID, "fault key row or word outside the call");
    }
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    u64 *part;
    if ((rc = sealed_scratch(ctx, st, p, false, &part))) return rc;
    kstep.flags_key = d_flags + lay[2];
    kstep.part = part;
    HIP_TRY(hipMemsetAsync(d_flags, 0, (size_t)lay[3] * sizeof(u32), st));
    uint64_t *d_report = rm ? reinterpret_cast<uint64_t *>(d_flags + report_offset(lay[4])) : nullptr;
    if (rm) HIP_TRY(hipMemsetAsync(d_report, 0, (size_t)lay[3] * 4 * sizeof(u64), st));      // rows without a seal report CLEAN
    const size_t L = p->L;
    const uint64_t *ops[2] = {d_c0, d_c1};
    for (int i = 0; i < 2; i++) {
        const SealedRows r{ops[i], d_seal_in ? d_seal_in[i] : nullptr, rm && rm->loc_in ? rm->loc_in[i] : nullptr, 1, L, lay[i]};
        if ((rc = verify_or_repair(st, p->t, r, d_flags, d_report, part))) return rc;
    }
    const SealedRows key{d_galois_key, d_seal_key, rm ? rm->loc_key : nullptr, (size_t)p->dnum * 2, L + p->K, lay[2]};
    if (!fused_key && (rc = verify_or_repair(st, p->t, key, d_flags, d_report, part))) return rc;
    if ((rc = checked(d_flags + lay[3]))) return rc;
    return seal_outputs(st, p->t, d_seal_out, rm ? rm->loc_out : nullptr, d_out0, d_out1, L, part);
}

int fhe_rotate_sealed(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1,
                      uint32_t galois_elt, const uint64_t *d_galois_key, const fhe_abft *a, const uint64_t *const *d_seal_in,
                      const uint64_t *d_seal_key, uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream)
{
    return rotate_sealed_body(nullptr, false, ctx, p, d_out0, d_out1, d_c0, d_c1, galois_elt, d_galois_key, a, d_seal_in, d_seal_key, d_seal_out, d_flags, stream);
}

int fhe_rotate_sealed_fused(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1,
                            uint32_t galois_elt, const uint64_t *d_galois_key, const fhe_abft *a, const uint64_t *const *d_seal_in,
                            const uint64_t *d_seal_key, uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream)
{
    return rotate_sealed_body(nullptr, true, ctx, p, d_out0, d_out1, d_c0, d_c1, galois_elt, d_galois_key, a, d_seal_in, d_seal_key, d_seal_out, d_flags, stream);
}

int fhe_rotate_sealed_repair_layout(const fhe_keyswitch *p, int out[8])
{
    int rc = fhe_rotate_sealed_layout(p, out);
    if (rc) return rc;
    out[5] = report_offset(out[4]);
    out[6] = out[5] + 8 * out[3];
    out[7] = 0;
    return FHE_OK;
}

int fhe_rotate_sealed_repair(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, uint64_t *d_c0, uint64_t *d_c1, uint32_t galois_elt,
                             uint64_t *d_galois_key, const fhe_abft *a, const uint64_t *const *d_seal_in, const uint64_t *const *d_locator_in,
                             const uint64_t *d_seal_key, const uint64_t *d_locator_key, uint64_t *const *d_seal_out, uint64_t *const *d_locator_out,
                             uint32_t *d_flags, void *stream)
{
    const RepairMode rm{d_locator_in, d_locator_key, d_locator_out};
    return rotate_sealed_body(&rm, false, ctx, p, d_out0, d_out1, d_c0, d_c1, galois_elt, d_galois_key, a, d_seal_in, d_seal_key, d_seal_out, d_flags, stream);
}

} // extern "C"
