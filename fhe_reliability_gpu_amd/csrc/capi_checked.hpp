// capi_checked.hpp -- what the stage-by-stage checked composites share (capi_keyswitch_checked.cpp: key switch, relinearisation,
// rotation; capi_hmult_checked.cpp: rescale / mod switch, homomorphic multiply; capi_rotate_hoisted_checked.cpp: the Galois
// permutation and hoisted rotations; capi_bsgs_checked.cpp: the BSGS matrix-vector product and the checked add;
// capi_bgv_checked.cpp: the checked scalar multiply; capi_seal.cpp: the sealed multiply and rotation): the flag layouts, the
// checked-transform helper over the plan's scratch sums, the scope and hook checks, and the checked key switch and rescale
// themselves.  The one-shot fault records are those of fault_hook.hpp.
//
// Each composite exists once and takes its form (KsForm) as a parameter: the CKKS form, or the BGV form of a plan with a plain
// modulus t, which is the same launch list plus two word-wise scalar stages (key switch: 9 and 10, mod switch: 4 and 5; numbered
// after the stages both forms share, 8 being the hoisted rotations' permutation).  The entry point chooses the form and names
// the context's hook record it takes -- fhe_*_checked the CKKS form, fhe_bgv_*_checked the BGV form, the sealed calls by the
// plan's plain modulus -- and the plan must agree with it (ksc_scope); the hoisted rotations and the BSGS product run the CKKS form.
#pragma once
#include "capi_internal.hpp"
#include "galois_check.hpp"

enum class KsForm { CKKS, BGV };
// the context's record an entry point takes its key-switch or rescale hook from: each form has records of its own
using KsHookSlot = StagedFault fhe_ctx::*;

// offsets by stage number; a stage the form does not have (8; 9 and 10 in the CKKS form) has no words
struct KscLayout {
    int off[11], total;
    int units(int stage) const { return (stage == 10 ? total : off[stage + 1]) - off[stage]; }
};
KscLayout ksc_layout(const fhe_keyswitch *p, KsForm form);

// slots of the plan's scratch sums, one per (polynomial, row) a stage's transforms address.  Key switch: stage 2 the dnum x M rows of
// ext, stage 4 rows L .. M-1 of both halves of acc ([2][M]: up to slot 2 M - 1), stage 6 [2][L], stage 0 [L].  Rescale: the residues
// of up to three parts, [3][L - 1] (more than the key switch needs on plans such as dnum = 1, K = 1, L > 5).
inline size_t ksc_slots(const fhe_keyswitch *p)
{
    return std::max((size_t)std::max(p->dnum, 2) * (p->L + p->K), (size_t)3 * std::max(p->L - 1, 0));
}

// the sealed inverse transform that opens a key switch (SealedSteps::in below) or a sealed product
struct SealedInputStep {
    const uint64_t *seal;          // DEVICE [L][2] the stored seals of d_c's rows, or null: not compared (the window still is)
    uint32_t *flags;               // the rows' flags, [L]: every word is written by stage 0
    u64 *part;                     // at least ntt_seal_part_words(L, log_n, true) words, not shared with a launch that runs before stage 0 ends
    u32 hit_row, hit_coeff;        // the sealed transform's hook, checked against the call (ntt_seal_hit); hit_mask == 0: not armed
    u64 hit_mask;
};

// the transforms of one checked stage: rows [row0, row0 + count) of n_poly polynomials `stride` rows apart inside base, row r on
// table limb tl0 + (r - row0); the sums of (polynomial, row) live at slot sum0 + polynomial * stride + row
struct KscRows {
    u64 *base;
    u32 row0, tl0, count, n_poly, stride, sum0;
};

struct KscNtt {
    const fhe_keyswitch *p;
    const fhe_abft *a;
    hipStream_t st;
    u32 tin, tout;
    bool inverse;
    u64 *sum_in() const { return p->chk_sum_in.as<u64>(); }
    u64 *sum_out() const { return p->chk_sum_out.as<u64>(); }

    int launch(const KscRows &r, int which) const
    {
        const fhe_ntt_tables *t = p->t;
        const size_t N = (size_t)1 << p->log_n;
        return for_each_run(t, r.count, r.tl0, [&](size_t off, size_t len, int path) -> int {
            PassArgs pa{r.base + (r.row0 + off) * N, t->d_lp.as<LimbParams>(), (u32)(r.tl0 + off), (u32)len, (u32)(r.n_poly * len), r.stride, nullptr};
            // the launch addresses slots slot + polynomial * stride + l, l < len
            const size_t slot = (size_t)r.sum0 + r.row0 + off;
            if (slot + (size_t)(r.n_poly - 1) * r.stride + len > ksc_slots(p)) return fail(FHE_ERR_INVALID, "checked call: a transform's sums lie outside the plan's scratch");
            hipError_t e = launch_ntt_checked(st, pa, a->win.as<Tw>(), a->wout.as<Tw>(), a->wout8.as<u64>(), sum_in() + slot * tin, sum_out() + slot * tout,
                                              p->log_n, path, which, inverse);
            return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_ntt_checked");
        });
    }
    // the inverse transform of one row range with its input's seal verified on the transform's own load (ntt_sealed.hip): out of
    // place from src (the rows as r addresses them inside src) into r.base, one polynomial; the rows' seal verdicts go to in.flags
    int launch_sealed(const KscRows &r, const u64 *src, const SealedInputStep &in, int which) const;
    int run_sealed(const KscRows &r, const u64 *src, const SealedInputStep &in, u64 *flip, int bit) const
    {
        int rc;
        if (!flip) return launch_sealed(r, src, in, -1);
        if ((rc = launch_sealed(r, src, in, 0))) return rc;
        hipError_t e = launch_flip_bit(st, flip, 0, bit);
        if (e != hipSuccess) return hip_fail(e, "launch_flip_bit");
        return launch_sealed(r, src, in, 1);
    }
    // all launches of the stage; flip != nullptr (test hook, two-launch sizes): that word is flipped between the stage's two launches
    int run(const std::vector<KscRows> &rows, u64 *flip, int bit) const
    {
        int rc;
        if (!flip) {
            for (const KscRows &r : rows)
                if ((rc = launch(r, -1))) return rc;
            return FHE_OK;
        }
        for (const KscRows &r : rows)
            if ((rc = launch(r, 0))) return rc;
        hipError_t e = launch_flip_bit(st, flip, 0, bit);
        if (e != hipSuccess) return hip_fail(e, "launch_flip_bit");
        for (const KscRows &r : rows)
            if ((rc = launch(r, 1))) return rc;
        return FHE_OK;
    }
    // flags[i] = sums of slot (slot0 + i) differ, i < units, unit i on table limb limb0 + i % limbs
    int compare(u32 *flags, u32 slot0, u32 limb0, u32 limbs, u32 units) const
    {
        if ((size_t)slot0 + units > ksc_slots(p)) return fail(FHE_ERR_INVALID, "checked call: a comparison's sums lie outside the plan's scratch");
        hipError_t e = launch_compare_sums(st, flags, sum_in() + (size_t)slot0 * tin, tin, sum_out() + (size_t)slot0 * tout, tout,
                                           p->t->d_lp.as<LimbParams>(), limb0, limbs, units);
        return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_compare_sums");
    }
};

// defined in capi_keyswitch_checked.cpp
// the flag map of stage 1, its job-order scratch and the detector's partial sums, once per plan
int ksc_prepare(fhe_keyswitch *p);
// the checked transforms of one direction; the detector's partial sums live in the plan (ksc_prepare): the fhe_abft is only read
KscNtt ksc_ntt(const fhe_keyswitch *p, const fhe_abft *a, hipStream_t st, bool inverse);
// scope of every stage-by-stage checked call: the plan, the detector and the context's transform variants.  The CKKS form refuses
// a plan with a plain modulus (FHE_ERR_UNSUPPORTED), the BGV form one without (FHE_ERR_INVALID) or with more than 64 limbs per
// scalar stage; mod_switch: the call drops a prime
int ksc_scope(const fhe_ctx *ctx, const fhe_keyswitch *p, const fhe_abft *a, const uint32_t *d_flags, KsForm form, bool mod_switch);
// a plan that rounds its rescale to nearest (fhe_keyswitch_set_rescale_rounding) has no checked, sealed or repairing form of a call
// that drops a prime: those restate the flooring words stage by stage and would floor silently.  Part of ksc_scope, so every such
// entry point refuses after taking its hooks and before its first launch; a call that drops no prime runs as on any other plan
inline int ksc_rounding_scope(const fhe_keyswitch *p, bool mod_switch)
{
    if (mod_switch && p->rescale_rounding)
        return fail(FHE_ERR_UNSUPPORTED, "the plan rounds its rescale to nearest: the checked and sealed rescales restate the flooring form (fhe_keyswitch_set_rescale_rounding)");
    return FHE_OK;
}

// ---- the sealed steps of a checked call: each replaces one launch of the checked call's list by its sealed form -- same words, same
// ABFT or residue flags at the same place -- and an absent step leaves that launch the checked call's own (SealedSteps below)
struct SealedKeyStep {
    const uint64_t *seal_key;      // DEVICE [dnum 2 M][2] the stored seals of the key's rows, or null: not compared
    uint32_t *flags_key;           // the key rows' flags, [dnum][2][M], zeroed by the caller
    u64 *part;                     // ctx->seal_part, at least ks_sealed_scratch_words(p) long
    KsSealHit hit;                 // the sealed call's hook, checked against the plan (ks_seal_hit)
};
struct SealedTailStep {
    uint64_t *seal_out[3];           // DEVICE [limbs][2] per output part, or null: that part is not sealed
    u64 *part;                       // at least subscale_seal_part_words(2 limbs, log_n, flags_in != nullptr) words
    int hit_point = -1;              // the sealed tail's hook, checked against the call (subscale_seal_hit): SS_AT_*, < 0: not armed
    u32 hit_part = 0, hit_limb = 0, hit_coeff = 0;
    u64 hit_mask = 0;
    // fhe_rescale_sealed alone: the rescale's input [n_parts][L] is verified on the loads that consume it -- rows below L - 1 on
    // stage 3's, the last limbs on stage 0's, which is then the sealed inverse transform out of place from the caller's rows
    const uint64_t *seal_in = nullptr;      // DEVICE [n_parts][L][2]
    uint32_t *flags_in = nullptr;           // [n_parts][L], zeroed by the caller
    u64 *part_ntt = nullptr;                // at least n_parts * ntt_seal_part_words(1, log_n, true) words, apart from `part`
    int ntt_hit_part = -1;                  // the sealed transform's hook, checked against the call: the part whose last limb it hits
    u32 ntt_hit_coeff = 0;
    u64 ntt_hit_mask = 0;
    // the record of one launch over output parts part0 and (two) part0 + 1 of `limbs` rows; L_in = rows per part of the sealed input
    SubScaleSeal launch(size_t part0, bool two, u32 limbs, u32 L_in) const
    {
        SubScaleSeal s{part, seal_out[part0], two ? seal_out[part0 + 1] : nullptr};
        if (flags_in) {
            s.seal_in = seal_in ? seal_in + 2 * part0 * L_in : nullptr;
            s.flags_in = flags_in + part0 * L_in;
            s.in_stride = L_in;
        }
        if (hit_point >= 0 && hit_part >= part0 && hit_part < part0 + (two ? 2 : 1)) {
            s.hit_point = hit_point;
            s.hit_row = (u32)(hit_part - part0) * limbs + hit_limb;
            s.hit_coeff = hit_coeff;
            s.hit_mask = hit_mask;
        }
        return s;
    }
    // does that launch have anything to verify or to seal (otherwise it is the checked launch)
    bool runs(size_t part0, bool two) const { return flags_in || seal_out[part0] || (two && seal_out[part0 + 1]); }
};
struct SealedTensorStep {
    const uint64_t *const *seal_in;      // HOST array of the seals of a0, a1, b0, b1; an entry or the array may be null
    uint32_t *flags_op[4];               // the operands' row flags, [L] each, zeroed by the caller
};
// the steps one call runs sealed, named by the caller that sets them; every checked body takes the record last and reads the steps of
// the launches it owns (ksc_front: in; ksc_back: key, tail; keyswitch_checked and rotate_checked: those three; hmult_checked: tensor,
// key, tail)
struct SealedSteps {
    // the multiply's tensor step is the sealed tensor product (tensor_sealed.hip) instead of fhe_tensor_product_checked: a0, a1, b0, b1
    // are verified on the load that multiplies them, and the call owns that step's hook (fhe_hmult_sealed_fused and above)
    const SealedTensorStep *tensor = nullptr;
    // stage 3 is the sealed inner product (mac_sealed.hip) instead of launch_ks_mac_checked: the key is verified on the load that
    // multiplies it (fhe_keyswitch_apply_sealed*, fhe_rotate_sealed_fused, _in, _out, fhe_hmult_sealed_fused_key, _out, the hoisted rotations)
    const SealedKeyStep *key = nullptr;
    // stage 0 is the sealed inverse transform (ntt_sealed.hip) out of place from d_c into the plan's coefficient buffer instead of the
    // copy followed by the checked inverse in place: d_c's seal is verified on the transform's own load (fhe_keyswitch_apply_sealed_in,
    // fhe_rotate_sealed_in, _out; capi_ntt_sealed.cpp)
    const SealedInputStep *in = nullptr;
    // the call's last launch -- the key switch's stage 7 when no rescale follows, the rescale's stage 3 otherwise -- is the sealed tail
    // (subscale_sealed.hip) instead of launch_sub_scale_checked: the outputs' seals are written from the registers it stores
    // (fhe_hmult_sealed_out, fhe_rotate_sealed_out, fhe_rescale_sealed; capi_subscale_sealed.cpp)
    const SealedTailStep *tail = nullptr;
};
int keyswitch_checked(fhe_keyswitch *p, KsForm form, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c, const uint64_t *d_evk,
                      const uint64_t *d_add0, const uint64_t *d_add1, const fhe_abft *a, uint32_t *d_flags, hipStream_t st, const StagedFault &ft,
                      const SealedSteps &steps = {});
// the whole rotation behind an entry point (fhe_rotate_checked, fhe_bgv_rotate_checked, fhe_rotate_sealed, fhe_rotate_sealed_fused),
// which has taken the form's key-switch hook: ft
int rotate_checked(KsForm form, const StagedFault &ft, fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0,
                   const uint64_t *d_c1, uint32_t galois_elt, const uint64_t *d_galois_key, const fhe_abft *a, uint32_t *d_flags, void *stream,
                   const SealedSteps &steps = {});

// ---- the checked key switch as two halves (keyswitch_checked = front + back; hoisted rotations: one front, a back per element)
// where each stage's flag words go: s[0..7] the stages of the key switch, s[8] the Galois permutation of a hoisted rotation, s[9]
// and s[10] the scalar stages of the BGV form (null in the CKKS form).  The caller clears them
struct KscFlags {
    u32 *s[11];
};
// a key-switch fault checked against the plan: the word a transform stage flips between its two launches, or the fault of a residue
// stage rebased to the launch it hits (block = the conversion job of stages 1 and 5: the digit, the half; unit = the unit inside
// that job's flags)
struct KscHook {
    StagedFault f;
    u64 *flip = nullptr;
};
int ksc_hook(const fhe_keyswitch *p, KsForm form, const StagedFault &ft, u64 *acc, bool has_add0, bool has_add1, KscHook &h);
// the permutation step of a hoisted rotation's back half: the sums ([2][M][N]) into acc_to, c0 ([L][N]) into c0_to
struct KscPerm {
    u32 galois_elt;
    const u64 *c0;
    u64 *acc_to, *c0_to;
    GaloisFault fault;       // unit = half * M + row for the sums, 2 M + l for c0
    // fhe_rotate_hoisted_sealed with c0's seal: the L rows of c0 go through the sealed permutation (galois_sealed.hip) instead, which
    // verifies them on its own gather -- their verdict lands in flags_c0 ([L], zeroed by the caller), their L words of the stage-8
    // block stay zero.  Null (every other call): c0 goes through the checked permutation with the sums
    const u64 *seal_c0 = nullptr;      // DEVICE [L][2]
    u32 *flags_c0 = nullptr;
    u64 *part = nullptr;               // at least galois_seal_part_words(L, log_n, false) long
    GalSealHit hit{-1, 0, 0, 0};       // the sealed permutation's hook, checked against the call
};
int ksc_front(fhe_keyswitch *p, const uint64_t *d_c, const fhe_abft *a, const KscFlags &fl, hipStream_t st, const KscHook &h,
              const SealedSteps &steps = {});
int ksc_back(fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c, const uint64_t *d_evk, const uint64_t *d_add0,
             const uint64_t *d_add1, const fhe_abft *a, const KscFlags &fl, hipStream_t st, const KscHook &h, const KscPerm *perm, KsForm form,
             const SealedSteps &steps = {});

// defined in capi_keyswitch_sealed.cpp
// does the plan take the fused route (dnum <= KS_SEAL_MAX_DNUM), or the sweep followed by the checked inner product
bool ks_sealed_fused(const fhe_keyswitch *p);
// words of ctx->seal_part the sealed stage needs on either route
size_t ks_sealed_scratch_words(const fhe_keyswitch *p);
// the sealed key switch's hook as a call took it (ctx->ks_seal_fault), checked against the plan: the key row and the word exist,
// and the plan takes the fused route (above the cap there is no fused load to hit)
int ks_seal_hit(const SealHook &f, const fhe_keyswitch *p, KsSealHit &hit);
// stage 3 of a key switch with a sealed key: the fused launch, or above the cap launch_seal_verify over the key's rows followed by
// launch_ks_mac_checked; k = the residue check record of stage 3, its flags [2][M]
int ks_mac_sealed_stage(const fhe_keyswitch *p, hipStream_t st, const KsMacArgs &ka, const BcCheck &k, const SealedKeyStep &key);

// defined in capi_ntt_fwd_sealed.cpp
// the sealed transform's hook as a call of `rows` rows took it (ctx->ntt_seal_fault), checked against that call
int ntt_seal_hit(const SealHook &f, size_t rows, int log_n, SealedInputStep &in);
// the sealed transform's record for the run of `len` limbs from limb `off` on, in a call of `limbs` limbs per polynomial whose input
// partials are `tin` per row
NttSealIn run_seal_in(const SealedInputStep &in, size_t off, size_t len, size_t limbs, u32 tin);

// defined in capi_bgv_checked.cpp
// one scalar stage: `limbs` rows from data on, of n_poly polynomials poly_stride rows apart (row l of polynomial i at data + (i
// poly_stride + l) N), times scal[l] mod q_(limb0 + l), in place (launch_scalar_affine_checked); flags [n_poly][limbs]
int bgv_scalar_stage(const fhe_keyswitch *p, hipStream_t st, u64 *data, const u64 *scal, u32 limb0, u32 limbs, u32 n_poly, u32 poly_stride, u32 *flags,
                     const StagedFault &f);

// defined in capi_hmult_checked.cpp
struct RscLayout {
    int off[6], total;
    int units(int stage) const { return (stage == 5 ? total : off[stage + 1]) - off[stage]; }
};
RscLayout rsc_layout(const fhe_keyswitch *p, size_t n_parts, KsForm form);
// the rescale's fault checked against the plan and the number of parts; *flip = the word a transform stage flips
int rsc_hook(const fhe_keyswitch *p, KsForm form, const StagedFault &ft, size_t n_parts, u64 **flip);
// d_in = [n_parts][L][N], outs[i] = [L - 1][N]; the caller has checked scope, arguments and overlap.  Clears the lay.total words
// at d_flags.  tail (the one step a rescale has, so passed as itself): stage 3 is the sealed tail, and with tail->flags_in stage 0 the sealed inverse transform
int rescale_checked(fhe_keyswitch *p, KsForm form, uint64_t *const *outs, const uint64_t *d_in, size_t n_parts, const fhe_abft *a, uint32_t *d_flags,
                    hipStream_t st, const StagedFault &ft, const SealedTailStep *tail = nullptr);
// the one-shot hooks a multiply owns whatever its outcome, taken by its entry point before the first refusal: the key switch's, the
// rescale's when it rescales, the tensor step's pointwise one, and the sealed tensor product's when that is the tensor step
struct HmultHooks {
    StagedFault ks, rs;
    PointFault pw;
    SealHook tensor;
};
HmultHooks hmult_take(fhe_ctx *ctx, KsHookSlot ks_hook, KsHookSlot rs_hook, int rescale, bool sealed_tensor);
// the multiply behind an entry point (fhe_hmult_checked, fhe_bgv_hmult_checked, the fhe_hmult_sealed* calls) and its layout
int hmult_checked_layout(const fhe_keyswitch *p, KsForm form, int rescale, int out[4]);
int hmult_checked(KsForm form, const HmultHooks &hk, fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_a0,
                  const uint64_t *d_a1, const uint64_t *d_b0, const uint64_t *d_b1, const uint64_t *d_relin_key, int rescale, const fhe_abft *a,
                  uint32_t *d_flags, void *stream, const SealedSteps &steps = {});

// defined in capi_subscale_sealed.cpp
// the sealed tail's hook as a call took it (ctx->subscale_seal_fault), checked against that call: in_rows_per_part != 0: the call
// runs the IN form over input parts of that many rows, of which the last is not read by the tail; out_limbs = rows per output part
// (0: the call has no output seals)
int subscale_seal_hit(const SealHook &f, size_t n_parts, size_t in_rows_per_part, size_t out_limbs, int log_n, SealedTailStep &tail);

// defined in capi_tensor_sealed.cpp
// the sealed tensor product's hook as a call of `units` rows took it (ctx->tensor_seal_fault), checked against that call
int tensor_seal_hit(const SealHook &f, size_t units, int log_n, TensorSealHit &hit);
// words of ctx->seal_part the sealed tensor product of `units` rows needs
size_t tensor_sealed_scratch_words(size_t units, int log_n, bool out);
// the launches of the sealed tensor product over rows [n_poly][limbs]: d = {d0, d1, d2}, ops = {a0, a1, b0, b1}, all 16-byte
// aligned and log_n >= 1 (the caller has checked both, the limb range and the hooks); seal_in / seal_out: HOST arrays as the entry
// point takes them; flags_op[o] = [rows], k.flags = [rows][3], all zeroed by the caller; grows ctx->seal_part where it is too small
int tensor_sealed_run(fhe_ctx *ctx, hipStream_t st, uint64_t *const d[3], const uint64_t *const ops[4], const fhe_ntt_tables *t, size_t n_poly, size_t limbs,
                      size_t start_idx, const uint64_t *const *seal_in, uint64_t *const *seal_out, uint32_t *const flags_op[4], const BcCheck &k,
                      const TensorSealHit &hit);

// defined in capi_rotate_hoisted_checked.cpp
// the checked permutation of up to two row ranges that share one flags array (units counted through the segments in order, the
// fault's unit too); the sums live in the context (grown on demand); every flag word is written
struct GalSeg {
    u64 *dst;
    const u64 *src;
    u32 units;
};
int galois_permute_checked(fhe_ctx *ctx, hipStream_t st, const GalSeg *segs, int n_segs, int logn, u32 galois_elt, u32 *d_flags, const GaloisFault &f);

// the checked hoisted rotations as a core (fhe_rotate_hoisted_checked; the baby block of fhe_bsgs_matvec_checked)
struct HrcLayout {
    int shared[3], rot[6];      // offsets of stages 0-2 in the shared block; of stages 3, 8, 4, 5, 6, 7 inside a rotation's block
    int n_shared, n_rot;        // words of the shared block, of one rotation's block
};
HrcLayout hrc_layout(const fhe_keyswitch *p);
// the hoisted rotations' fault (block = the rotation) checked against the plan and the number of rotations
struct HrcHook {
    int stage = -1, rot = 0;
    KscHook hook;            // stages 0-7
    GaloisFault gal;         // stage 8
};
int galois_fault_check(const GaloisFault &f, size_t units, int logn);
// the plan's buffers (partial sums, second set of sums) and the hook's validation: before anything is launched
int hrc_prepare(fhe_keyswitch *p, const StagedFault &ft, size_t n_rot, HrcHook &h);
// fhe_rotate_hoisted_sealed's additions to the launch list (capi_galois_sealed.cpp); absent, hrc_run's list is what it was.  Rotation
// r's input flags are flags_in + r * stride: [c0 rows L][key rows dnum 2 M], zeroed by the caller.  Stage 3 runs through a
// SealedKeyStep with seal_keys[r]; c0 through the sealed permutation when seal_c0 is given
struct HrcSealed {
    const uint64_t *seal_c0;               // DEVICE [L][2], or null: c0 goes through the checked permutation
    const uint64_t *const *seal_keys;      // HOST [n_rot] of DEVICE [dnum 2 M][2]; the array or an entry may be null
    u32 *flags_in;
    size_t stride;
    u64 *part;                             // ctx->seal_part, long enough for the key step and the sealed permutation
    GalSealHit hit;                        // the sealed permutation's hook, for rotation hit_rot
    size_t hit_rot;
};
// the launches; d_flags = the shared block then one block per rotation (hrc_layout), cleared by the caller
int hrc_run(fhe_keyswitch *p, uint64_t *const *d_out0, uint64_t *const *d_out1, const uint64_t *d_c0, const uint64_t *d_c1, const uint32_t *galois_elts,
            const uint64_t *const *d_prepared_keys, size_t n_rot, const fhe_abft *a, uint32_t *d_flags, hipStream_t st, const HrcHook &h,
            const HrcSealed *sealed = nullptr);
