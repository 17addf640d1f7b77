// capi_sealed.hpp -- what the sealed entry points share (capi_seal.cpp, capi_seal_carry.cpp, capi_tensor_sealed.cpp,
// capi_keyswitch_sealed.cpp, capi_galois_sealed.cpp, capi_ntt_sealed.cpp, capi_ntt_fwd_sealed.cpp, capi_polymul_sealed.cpp,
// capi_subscale_sealed.cpp, capi_bsgs_checked.cpp, capi_abft.cpp): the alignment test, the context's partial-sum scratch, the form a plan runs, the
// flag layout and the prologue of the sealed key-switch calls, and the sweeps that verify given seals and seal outputs.  Host only.
#pragma once
#include "capi_checked.hpp"
#include "seal_check.hpp"

#include <cstdint>
#include <initializer_list>

// sealed rows are read 16 bytes at a time (a null pointer passes)
inline bool misaligned(std::initializer_list<const void *> ptrs)
{
    for (const void *q : ptrs)
        if ((uintptr_t)q % 16) return true;
    return false;
}

// the partial-sum scratch of the context, at least `words` long.  Growing frees the old block, which launches in flight on st may
// still read: the stream is drained first (once per context and shape)
inline int seal_scratch(fhe_ctx *ctx, hipStream_t st, size_t words, u64 **out)
{
    if (ctx->seal_part.bytes < words * 8) {
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(ctx->seal_part.alloc(words * 8));
    }
    *out = ctx->seal_part.as<u64>();
    return FHE_OK;
}

// the six partial-sum arrays of a checked product of `units` rows in the detector's psum (grown on demand, the stream drained first),
// laid out as fhe_polymul_checked lays them out; s.t_in / t_mid / t_out are set by the caller.  Squaring: one forward transform,
// both checks read its input sums
inline int polymul_sums(fhe_abft *m, hipStream_t st, size_t units, bool square, PolymulSums &s)
{
    const size_t words = units * (2 * s.t_in + 3 * s.t_mid + s.t_out);
    if (m->psum.bytes < words * 8) {
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(m->psum.alloc(words * 16));
    }
    s.ain = m->psum.as<u64>();
    s.bin = s.ain + units * s.t_in;
    s.aout = s.bin + units * s.t_in;
    s.bout = s.aout + units * s.t_mid;
    s.cin = s.bout + units * s.t_mid;
    s.cout = s.cin + units * s.t_mid;
    if (square) s.bin = s.ain;
    return FHE_OK;
}
// a launch's rows of those sums: row o of the call on
inline void polymul_sums_from(PolymulSums &r, size_t o)
{
    r.ain += o * r.t_in, r.bin += o * r.t_in, r.aout += o * r.t_mid, r.bout += o * r.t_mid, r.cin += o * r.t_mid, r.cout += o * r.t_out;
}

// rows of a switching key, [dnum][2][M]
inline size_t key_rows(const fhe_keyswitch *p) { return (size_t)p->dnum * 2 * (p->L + p->K); }

// the form of the checked call a sealed call runs -- by the plan's plain modulus -- with that form's hook records
struct SealedForm {
    KsForm form;
    KsHookSlot ks_hook, rs_hook;
};
inline SealedForm sealed_form(const fhe_keyswitch *p)
{
    if (p && p->plain_modulus) return SealedForm{KsForm::BGV, &fhe_ctx::bgv_ksc_fault, &fhe_ctx::bgv_rsc_fault};
    return SealedForm{KsForm::CKKS, &fhe_ctx::ksc_fault, &fhe_ctx::rsc_fault};
}

// the flag layout every sealed key-switch call shares -- k input blocks of L rows, the key's rows, the checked call's block of
// `checked` words: out[0 .. k - 1] the inputs, out[k] the key, out[k + 1] the checked block, out[k + 2] the total.  Returns k + 3,
// the index of the word the caller closes the layout with
inline int sealed_layout(const fhe_keyswitch *p, int k, int checked, int *out)
{
    for (int i = 0; i <= k; i++) out[i] = i * p->L;
    out[k + 1] = out[k] + (int)key_rows(p);
    out[k + 2] = out[k + 1] + checked;
    return k + 3;
}
// that layout around the checked key switch, as a layout call: closed by "the plan takes the fused route" (fused_word), or by 0
inline int ks_sealed_layout(const fhe_keyswitch *p, int k, bool fused_word, int *out)
{
    if (!p || !out) return fail(FHE_ERR_INVALID, "null argument");
    out[sealed_layout(p, k, ksc_layout(p, sealed_form(p).form).total, out)] = fused_word && ks_sealed_fused(p);
    return FHE_OK;
}

// ---- the key-switch family (fhe_keyswitch_apply_sealed, fhe_keyswitch_apply_sealed_in, fhe_rotate_sealed_in, fhe_rotate_sealed_out):
// one prologue and one call of keyswitch_checked, both defined in capi_keyswitch_sealed.cpp
// what a rotation of the family adds to the key switch it ends in; `out`: the tail seals the outputs (fhe_rotate_sealed_out)
struct KsSealedRotation {
    uint32_t galois_elt;
    const uint64_t *const *d_seal_in;      // the seals of c0 and c1, both required
    uint64_t *const *d_seal_out;
    bool out;
};
// the call as its entry point takes it.  A rotation switches sigma(c1) with sigma(c0) as the first addend: d_c = c1, d_evk = the
// Galois key, d_add0 = c0 (required), d_add1 = null
struct KsSealedCall {
    fhe_ctx *ctx;
    fhe_keyswitch *p;
    uint64_t *d_out0, *d_out1;
    const uint64_t *d_c, *d_evk, *d_add0, *d_add1;
    const fhe_abft *a;
    const uint64_t *d_seal_key;
    uint32_t *d_flags;
    void *stream;
    int in_blocks;                   // blocks of L input flag words before the key's: 0, 1 (c: _apply_sealed_in), 3 (c0, c1, sigma(c1): rot)
    const uint64_t *d_seal_c;        // in_blocks == 1: the seal of d_c, required
    const KsSealedRotation *rot;     // in_blocks == 3
};
// the call between its prologue and keyswitch_checked
struct KsSealed {
    KsForm form;
    StagedFault ft;                  // the form's key-switch hook
    hipStream_t st;
    int lay[7];                      // ks_sealed_layout(p, in_blocks)
    u64 *part, *behind;              // the launches' shared partials (stream order keeps them apart); rotation: 2 L words behind them
    SealedKeyStep key;
    SealedInputStep in;              // in_blocks != 0; its flags are the last input block
    SealedTailStep tail;             // rot->out
};
// the prologue, in this order: every hook of the steps the call runs is taken (they belong to it whatever its outcome); a missing
// d_seal_c; scope; null, missing-seal (rotation), identical-output, Galois-element and alignment refusals; the sealed steps' hooks
// against the call; ksc_prepare and the checked key switch's hook against the call; the scratch; the clear of the input and key flags
int ks_sealed_open(const KsSealedCall &c, KsSealed &k);
// keyswitch_checked on d_c with first addend d_add0 (the call's own, or a rotation's sigma(c1) and sigma(c0)) and the steps k holds
int ks_sealed_run(const KsSealedCall &c, const KsSealed &k, const uint64_t *d_c, const uint64_t *d_add0);

// rows [n_poly][limbs] of table set t from limb start_idx on
inline SealArgs seal_args(const fhe_ntt_tables *t, const uint64_t *d_words, size_t n_poly, size_t limbs, size_t start_idx)
{
    return SealArgs{d_words, t->d_lp.as<LimbParams>(), (u32)start_idx, (u32)limbs, (u32)(n_poly * limbs), (u32)limbs, t->log_n};
}

// the rows against their seal, verdicts at flags (zeroed by the caller); a null seal is skipped.  hook: the sweep's own fault
inline int verify_rows(hipStream_t st, const SealArgs &sa, const uint64_t *seal, u32 *flags, u64 *part, const BcCheck *hook = nullptr)
{
    if (!seal) return FHE_OK;
    BcCheck k = hook ? *hook : BcCheck{nullptr, -1, 0, 0, 0};
    k.flags = flags;
    hipError_t e = launch_seal_verify(st, sa, part, seal, k);
    return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_seal_verify");
}

// seals and locators of the two outputs, `limbs` rows each from limb 0 on, where a buffer was given (either array may be null)
inline int seal_outputs(hipStream_t st, const fhe_ntt_tables *t, uint64_t *const *d_seal_out, uint64_t *const *d_loc_out, const uint64_t *d_out0,
                        const uint64_t *d_out1, size_t limbs, u64 *part)
{
    const uint64_t *outs[2] = {d_out0, d_out1};
    for (int h = 0; h < 2; h++) {
        const SealArgs sa = seal_args(t, outs[h], 1, limbs, 0);
        if (d_seal_out && d_seal_out[h]) {
            hipError_t e = launch_seal(st, sa, part, d_seal_out[h], BcCheck{nullptr, -1, 0, 0, 0});
            if (e != hipSuccess) return hip_fail(e, "launch_seal");
        }
        if (d_loc_out && d_loc_out[h]) {
            hipError_t e = launch_seal_locator(st, sa, part, d_loc_out[h]);
            if (e != hipSuccess) return hip_fail(e, "launch_seal_locator");
        }
    }
    return FHE_OK;
}

// a row hook (unit = the row, coeff = the word) as a launch of `units` rows took it, checked against that launch: fires at `point`
inline int row_fault(const PointFault &f, int point, size_t units, int log_n, BcCheck &k)
{
    if (f.point < 0) return FHE_OK;
    if (f.unit >= units || f.coeff >> log_n) return fail(FHE_ERR_INVALID, "fault row or word outside the call");
    k.fault_point = point;
    k.fault_unit = f.unit;
    k.fault_coeff = f.coeff;
    k.fault_mask = (u64)1 << f.bit;
    return FHE_OK;
}
