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

// how much of a sweep-based composite rides on the loads that consume the data instead of sweeps of its own; each level keeps what
// the one before it fused.  A repairing call (RepairMode) runs at Sweep: repair needs the sweep
enum class SealedLevel {
    Sweep,             // every given seal verified by a sweep of its own, both outputs sealed by sweeps
    Tensor,            // the multiply's four operand sweeps are gone: its tensor step is the sealed tensor product (capi_tensor_sealed.cpp),
                       // which verifies a0, a1, b0, b1 on the load that multiplies them and writes their row flags where the sweeps wrote them
    TensorKey,         // the key's sweep is gone as well: the key switch's inner product is the sealed one (capi_keyswitch_sealed.cpp), which
                       // writes the key rows' flags where the sweep wrote them; the call takes that step's hook.  (A rotation has no tensor
                       // step: the sweeps over c0 and c1 stay)
    TensorKeyOut,      // the two output sweeps are gone as well: the call's last launch is the sealed tail (capi_subscale_sealed.cpp), which
                       // writes the outputs' seals from the registers it stores; the call takes that step's hook
};

// one sweep-based composite as its entry point describes it; the entry point has taken the checked call's own hooks
struct SealedCall {
    fhe_ctx *ctx;
    fhe_keyswitch *p;
    uint64_t *d_out0, *d_out1;
    int n_ops;
    const uint64_t *ops[4];              // the operands in flag order, L rows each
    const uint64_t *d_key;
    int rescale;                         // the multiply drops a prime: outputs of L - 1 rows
    const SealHook *tensor_hook;         // the sealed tensor product's hook as the multiply took it; null: the checked call has no tensor step
    bool refused;                        // what else the checked call refuses before its first launch (an even Galois element)
    const fhe_abft *a;
    const uint64_t *const *d_seal_in;
    const uint64_t *d_seal_key;
    uint64_t *const *d_seal_out;
    uint32_t *d_flags;
    void *stream;
    int (*checked_words)(const fhe_keyswitch *p, KsForm form, int rescale);      // words of the checked call's own block
};

// the body of every sweep-based composite; checked(flags, steps) runs the checked call with the hooks its entry point took.  Every
// hook the call owns is taken before the first refusal.  Refusals, in order: scope and the arguments the checked call refuses (its
// status and message), alignment, an unpaired seal and locator, then the sealed steps' hooks against the call (tensor, key, tail)
template <class Checked>
int sealed_composite(const RepairMode *rm, SealedLevel level, const SealedCall &c, KsForm form, Checked checked)
{
    if (rm && level != SealedLevel::Sweep) return fail(FHE_ERR_INVALID, "a repairing call runs the sweeps");
    fhe_ctx *ctx = c.ctx;
    fhe_keyswitch *p = c.p;
    uint32_t *d_flags = c.d_flags;
    const int n = c.n_ops;
    const bool fused_ops = level >= SealedLevel::Tensor && c.tensor_hook, fused_key = level >= SealedLevel::TensorKey, out = level >= SealedLevel::TensorKeyOut;
    const SealHook kf = fused_key ? ctx->ks_seal_fault.take() : SealHook{};      // one shot, whatever the outcome
    const SealHook tf = out ? ctx->subscale_seal_fault.take() : SealHook{};
    SealedTensorStep tstep{c.d_seal_in, {nullptr, nullptr, nullptr, nullptr}};
    SealedKeyStep kstep{c.d_seal_key, nullptr, nullptr, KsSealHit{0, 0, 0}};
    SealedTailStep tail{{c.d_seal_out ? c.d_seal_out[0] : nullptr, c.d_seal_out ? c.d_seal_out[1] : nullptr, nullptr}, nullptr};
    SealedSteps steps;
    if (fused_ops) steps.tensor = &tstep;
    if (fused_key) steps.key = &kstep;
    if (out) steps.tail = &tail;
    // what must hold before the first verifying launch, so that a call outside the checked call's scope launches nothing: the
    // checked call itself then refuses, and its status and message are the call's
    bool bad = c.refused || !c.d_out0 || !c.d_out1 || c.d_out0 == c.d_out1 || !c.d_key;
    for (int i = 0; i < n; i++) bad = bad || !c.ops[i];
    if (ksc_scope(ctx, p, c.a, d_flags, form, c.rescale != 0) || bad) {
        const int rc = checked(d_flags, steps);
        return rc ? rc : fail(FHE_ERR_INVALID, "sealed call: bad argument");
    }
    if (misaligned({c.d_out0, c.d_out1, c.ops[0], c.ops[1], c.ops[2], c.ops[3], c.d_key, rm ? d_flags : nullptr}))
        return fail(FHE_ERR_INVALID, "sealed rows are read 16 bytes at a time: the buffers must be 16-byte aligned");
    if (unpaired(rm, c.d_seal_in, n, c.d_seal_key)) return fail(FHE_ERR_INVALID, "a repairing call takes an operand's seal and locator together");
    int lay[8], rc;
    sealed_layout(p, n, c.checked_words(p, form, c.rescale), lay);      // lay[i] operand i, lay[n] the key, lay[n + 1] the checked block, lay[n + 2] the total
    const size_t L = p->L, out_limbs = c.rescale ? L - 1 : L;
    if (fused_ops) {
        TensorSealHit hit;
        if ((rc = tensor_seal_hit(*c.tensor_hook, L, p->log_n, hit))) return rc;
        for (int i = 0; i < n; i++) tstep.flags_op[i] = d_flags + lay[i];
    }
    if (fused_key && ks_seal_hit(kf, p, kstep.hit)) return fail(FHE_ERR_INVALID, "fault key row or word outside the call");
    if (out && (rc = subscale_seal_hit(tf, 2, 0, tail.seal_out[0] && tail.seal_out[1] ? out_limbs : 0, p->log_n, tail))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, c.stream);
    u64 *part;
    if ((rc = sealed_scratch(ctx, st, p, fused_ops, &part))) return rc;
    kstep.flags_key = d_flags + lay[n];
    kstep.part = tail.part = part;      // the key's verdict is out before the tail starts on the same stream
    HIP_TRY(hipMemsetAsync(d_flags, 0, (size_t)lay[n + 1] * sizeof(u32), st));
    uint64_t *d_report = rm ? reinterpret_cast<uint64_t *>(d_flags + report_offset(lay[n + 2])) : nullptr;
    if (rm) HIP_TRY(hipMemsetAsync(d_report, 0, (size_t)lay[n + 1] * 4 * sizeof(u64), st));      // rows without a seal report CLEAN
    for (int i = 0; i < n && !fused_ops; i++) {
        const SealedRows r{c.ops[i], c.d_seal_in ? c.d_seal_in[i] : nullptr, rm && rm->loc_in ? rm->loc_in[i] : nullptr, 1, L, lay[i]};
        if ((rc = verify_or_repair(st, p->t, r, d_flags, d_report, part))) return rc;
    }
    const SealedRows key{c.d_key, c.d_seal_key, rm ? rm->loc_key : nullptr, (size_t)p->dnum * 2, L + p->K, lay[n]};
    if (!fused_key && (rc = verify_or_repair(st, p->t, key, d_flags, d_report, part))) return rc;
    if ((rc = checked(d_flags + lay[n + 1], steps)) || out) return rc;
    return seal_outputs(st, p->t, c.d_seal_out, rm ? rm->loc_out : nullptr, c.d_out0, c.d_out1, out_limbs, part);
}

// the ten sealed multiplies and rotations: the form by the plan's plain modulus, the checked call's hooks taken here
int hmult_sealed(const RepairMode *rm, SealedLevel level, fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_a0,
                 const uint64_t *d_a1, const uint64_t *d_b0, const uint64_t *d_b1, const uint64_t *d_relin_key, int rescale, const fhe_abft *a,
                 const uint64_t *const *d_seal_in, const uint64_t *d_seal_key, uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    const SealedForm f = sealed_form(p);
    const HmultHooks hk = hmult_take(ctx, f.ks_hook, f.rs_hook, rescale, level >= SealedLevel::Tensor);
    const SealedCall c{ctx, p, d_out0, d_out1, 4, {d_a0, d_a1, d_b0, d_b1}, d_relin_key, rescale, &hk.tensor, false, a, d_seal_in, d_seal_key, d_seal_out, d_flags, stream,
                       [](const fhe_keyswitch *q, KsForm form, int rs) { int in[4] = {}; return hmult_checked_layout(q, form, rs, in) ? 0 : in[3]; }};
    return sealed_composite(rm, level, c, f.form, [&](uint32_t *flags, const SealedSteps &steps) {
        return hmult_checked(f.form, hk, ctx, p, d_out0, d_out1, d_a0, d_a1, d_b0, d_b1, d_relin_key, rescale, a, flags, stream, steps);
    });
}

int rotate_sealed(const RepairMode *rm, SealedLevel level, fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0,
                  const uint64_t *d_c1, uint32_t galois_elt, const uint64_t *d_galois_key, const fhe_abft *a, const uint64_t *const *d_seal_in,
                  const uint64_t *d_seal_key, uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    const SealedForm f = sealed_form(p);
    const StagedFault ft = (ctx->*f.ks_hook).take();
    const SealedCall c{ctx, p, d_out0, d_out1, 2, {d_c0, d_c1, nullptr, nullptr}, d_galois_key, 0, nullptr, !(galois_elt & 1), a, d_seal_in, d_seal_key, d_seal_out, d_flags, stream,
                       [](const fhe_keyswitch *q, KsForm form, int) { return ksc_layout(q, form).total; }};
    return sealed_composite(rm, level, c, f.form, [&](uint32_t *flags, const SealedSteps &steps) {
        return rotate_checked(f.form, ft, ctx, p, d_out0, d_out1, d_c0, d_c1, galois_elt, d_galois_key, a, flags, stream, steps);
    });
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
    out[sealed_layout(p, 4, inner[3], out)] = 0;
    return FHE_OK;
}

int fhe_hmult_sealed(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_a0, const uint64_t *d_a1,
    const uint64_t *d_b0, const uint64_t *d_b1, const uint64_t *d_relin_key, int rescale, const fhe_abft *a,
    const uint64_t *const *d_seal_in, const uint64_t *d_seal_key, uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream)
{
    return hmult_sealed(nullptr, SealedLevel::Sweep, ctx, p, d_out0, d_out1, d_a0, d_a1, d_b0, d_b1, d_relin_key, rescale, a, d_seal_in, d_seal_key, d_seal_out, d_flags, stream);
}

int fhe_hmult_sealed_fused(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_a0, const uint64_t *d_a1,
    const uint64_t *d_b0, const uint64_t *d_b1, const uint64_t *d_relin_key, int rescale, const fhe_abft *a,
    const uint64_t *const *d_seal_in, const uint64_t *d_seal_key, uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream)
{
    return hmult_sealed(nullptr, SealedLevel::Tensor, ctx, p, d_out0, d_out1, d_a0, d_a1, d_b0, d_b1, d_relin_key, rescale, a, d_seal_in, d_seal_key, d_seal_out, d_flags, stream);
}

int fhe_hmult_sealed_fused_key(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_a0, const uint64_t *d_a1,
    const uint64_t *d_b0, const uint64_t *d_b1, const uint64_t *d_relin_key, int rescale, const fhe_abft *a,
    const uint64_t *const *d_seal_in, const uint64_t *d_seal_key, uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream)
{
    return hmult_sealed(nullptr, SealedLevel::TensorKey, ctx, p, d_out0, d_out1, d_a0, d_a1, d_b0, d_b1, d_relin_key, rescale, a, d_seal_in, d_seal_key, d_seal_out, d_flags, stream);
}

int fhe_hmult_sealed_out(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_a0, const uint64_t *d_a1,
    const uint64_t *d_b0, const uint64_t *d_b1, const uint64_t *d_relin_key, int rescale, const fhe_abft *a,
    const uint64_t *const *d_seal_in, const uint64_t *d_seal_key, uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream)
{
    return hmult_sealed(nullptr, SealedLevel::TensorKeyOut, ctx, p, d_out0, d_out1, d_a0, d_a1, d_b0, d_b1, d_relin_key, rescale, a, d_seal_in, d_seal_key, d_seal_out, d_flags, stream);
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
    return hmult_sealed(&rm, SealedLevel::Sweep, ctx, p, d_out0, d_out1, d_a0, d_a1, d_b0, d_b1, d_relin_key, rescale, a, d_seal_in, d_seal_key, d_seal_out, d_flags, stream);
}

int fhe_rotate_sealed_layout(const fhe_keyswitch *p, int out[6]) { return ks_sealed_layout(p, 2, false, out); }

int fhe_rotate_sealed(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1,
    uint32_t galois_elt, const uint64_t *d_galois_key, const fhe_abft *a, const uint64_t *const *d_seal_in,
    const uint64_t *d_seal_key, uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream)
{
    return rotate_sealed(nullptr, SealedLevel::Sweep, ctx, p, d_out0, d_out1, d_c0, d_c1, galois_elt, d_galois_key, a, d_seal_in, d_seal_key, d_seal_out, d_flags, stream);
}

int fhe_rotate_sealed_fused(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1,
    uint32_t galois_elt, const uint64_t *d_galois_key, const fhe_abft *a, const uint64_t *const *d_seal_in,
    const uint64_t *d_seal_key, uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream)
{
    return rotate_sealed(nullptr, SealedLevel::TensorKey, ctx, p, d_out0, d_out1, d_c0, d_c1, galois_elt, d_galois_key, a, d_seal_in, d_seal_key, d_seal_out, d_flags, stream);
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
    return rotate_sealed(&rm, SealedLevel::Sweep, ctx, p, d_out0, d_out1, d_c0, d_c1, galois_elt, d_galois_key, a, d_seal_in, d_seal_key, d_seal_out, d_flags, stream);
}

} // extern "C"
