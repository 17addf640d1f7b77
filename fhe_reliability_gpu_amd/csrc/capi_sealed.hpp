// capi_sealed.hpp -- what the sealed entry points share (capi_seal.cpp, capi_seal_carry.cpp, capi_tensor_sealed.cpp,
// capi_keyswitch_sealed.cpp, capi_galois_sealed.cpp, capi_ntt_sealed.cpp, capi_bsgs_checked.cpp): the alignment test, the context's
// partial-sum scratch, the form a plan runs, and the sweeps that verify given seals and seal outputs.  Host only.
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
