// capi_keyswitch_sealed.cpp -- the key switch with the switching key verified on the load that multiplies it (mac_seal.hpp,
// mac_sealed.hip): fhe_keyswitch_apply_sealed, its layout and its test hook (part of the C ABI of include/fhe_mi355x.h), and
// the sealed stage 3 behind them as a step of a composite (fhe_rotate_sealed_fused, fhe_hmult_sealed_fused_key, capi_seal.cpp).
//
// The sealed composites verify the key's rows in a sweep of their own and the checked key switch multiplies from a second load.
// Here the inner product loads every key word once, digests it from the register that is handed to the product, and a finish
// launch holds the rows' sums against the stored seal.  The flag buffer of fhe_keyswitch_apply_sealed is
//     [key rows, [dnum][2][M]][the checked key switch's own block, exactly its layout]
// and a raised key flag does not stop the call: the words are the product of the key as it was loaded, and the residue identity
// holds on them.  The ciphertext d_c is not sealed here: its consuming loads are inside the transform kernels of stage 0.
//
// Above KS_SEAL_MAX_DNUM digits there is no fused instantiation: the stage is then the verifying sweep over the key's rows followed
// by the checked inner product, writing the same flag words (a key without a stored seal is then not swept at all, as in the
// sweep-based composites; on the fused route its window is checked all the same).
#include "capi_sealed.hpp"
#include "mac_seal.hpp"

bool ks_sealed_fused(const fhe_keyswitch *p) { return p->dnum >= 1 && (u32)p->dnum <= KS_SEAL_MAX_DNUM && p->log_n >= 1; }

// either route: the partials of the fused launch are [M][chunks][2 dnum][2], those of the sweep [dnum 2 M][chunks][2]
size_t ks_sealed_scratch_words(const fhe_keyswitch *p)
{
    return std::max(ks_seal_part_words((u32)(p->L + p->K), p->log_n, (u32)p->dnum), seal_part_words((u32)key_rows(p), p->log_n));
}

int ks_seal_hit(const SealHook &f, const fhe_keyswitch *p, KsSealHit &hit)
{
    hit = KsSealHit{0, 0, 0};
    if (f.sel < 0) return FHE_OK;
    if (!f.inside(key_rows(p), p->log_n)) return fail(FHE_ERR_INVALID, "fault key row or word outside the call");
    if (!ks_sealed_fused(p)) return fail(FHE_ERR_INVALID, "fault outside the call: above the fused cap no load of the inner product digests the key");
    hit = KsSealHit{(u32)f.row, (u64)f.coeff, (u64)1 << f.bit};
    return FHE_OK;
}

int ks_mac_sealed_stage(const fhe_keyswitch *p, hipStream_t st, const KsMacArgs &ka, const BcCheck &k, const SealedKeyStep &key)
{
    hipError_t e;
    if (ks_sealed_fused(p)) {
        e = launch_ks_mac_sealed(st, ka, key.part, key.seal_key, key.flags_key, k, key.hit);
        return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_ks_mac_sealed");
    }
    const int rc = verify_rows(st, seal_args(p->t, ka.evk, (size_t)p->dnum * 2, ka.M, 0), key.seal_key, key.flags_key, key.part);
    if (rc) return rc;
    e = launch_ks_mac_checked(st, ka, k);
    return e == hipSuccess ? FHE_OK : hip_fail(e, "launch_ks_mac_checked");
}

extern "C" {

int fhe_ctx_inject_fault_keyswitch_sealed(fhe_ctx *ctx, int key_row, long long coeff, int bit)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    return ctx->ks_seal_fault.arm(INT_MAX, key_row, 0, key_row, coeff, bit) ? FHE_OK : fail(FHE_ERR_INVALID, "bad fault");
}

int fhe_keyswitch_sealed_layout(const fhe_keyswitch *p, int out[4]) { return ks_sealed_layout(p, 0, true, out); }

int fhe_keyswitch_apply_sealed(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c, const uint64_t *d_evk,
                               const uint64_t *d_add0, const uint64_t *d_add1, const fhe_abft *a, const uint64_t *d_seal_key, uint32_t *d_flags, void *stream)
{
    const KsSealedCall c{ctx, p, d_out0, d_out1, d_c, d_evk, d_add0, d_add1, a, d_seal_key, d_flags, stream, 0, nullptr, nullptr};
    KsSealed k;
    const int rc = ks_sealed_open(c, k);
    return rc ? rc : ks_sealed_run(c, k, d_c, d_add0);
}

} // extern "C"

int ks_sealed_open(const KsSealedCall &c, KsSealed &k)
{
    fhe_ctx *ctx = c.ctx;
    fhe_keyswitch *p = c.p;
    const KsSealedRotation *rot = c.rot;
    const int nb = c.in_blocks;
    if (!ctx) return fail(FHE_ERR_INVALID, "null ctx");
    const SealedForm f = sealed_form(p);
    k.form = f.form;
    k.ft = (ctx->*f.ks_hook).take();
    const SealHook kf = ctx->ks_seal_fault.take();
    const SealHook nf = nb ? ctx->ntt_seal_fault.take() : SealHook{};
    const SealHook tf = rot && rot->out ? ctx->subscale_seal_fault.take() : SealHook{};
    // (the key switch refuses a missing input seal before scope, the rotation after the null arguments)
    if (nb == 1 && !c.d_seal_c) return fail(FHE_ERR_INVALID, "null d_seal_c: nothing would verify the input limbs (fhe_keyswitch_apply_sealed takes none)");
    int rc = ksc_scope(ctx, p, c.a, c.d_flags, k.form, false);
    if (rc) return rc;
    if (!c.d_out0 || !c.d_out1 || !c.d_c || !c.d_evk || (rot && !c.d_add0)) return fail(FHE_ERR_INVALID, "null argument");
    if (rot && (!rot->d_seal_in || !rot->d_seal_in[0] || !rot->d_seal_in[1]))
        return fail(FHE_ERR_INVALID, "null seal of c0 or c1: nothing would verify the permutation's source");
    if (c.d_out0 == c.d_out1) return fail(FHE_ERR_INVALID, "the two output parts must be distinct buffers");
    if (rot && !(rot->galois_elt & 1)) return fail(FHE_ERR_INVALID, "Galois elements are odd");
    if (rot && p->log_n < 1) return fail(FHE_ERR_UNSUPPORTED, "a sealed row has at least two words");
    if (misaligned({c.d_out0, c.d_out1, c.d_c, c.d_evk, c.d_add0, c.d_add1}))
        return fail(FHE_ERR_INVALID, "sealed rows are read 16 bytes at a time: the buffers must be 16-byte aligned");
    if ((rc = ks_sealed_layout(p, nb, true, k.lay))) return rc;
    const size_t L = (size_t)p->L;
    k.key = SealedKeyStep{c.d_seal_key, c.d_flags + k.lay[nb], nullptr, KsSealHit{0, 0, 0}};
    k.in = SealedInputStep{c.d_seal_c, c.d_flags + k.lay[nb ? nb - 1 : 0], nullptr, 0, 0, 0};
    k.tail = SealedTailStep{{rot && rot->d_seal_out ? rot->d_seal_out[0] : nullptr, rot && rot->d_seal_out ? rot->d_seal_out[1] : nullptr, nullptr}, nullptr};
    if ((rc = ks_seal_hit(kf, p, k.key.hit))) return rc;
    if (nb && (rc = ntt_seal_hit(nf, L, p->log_n, k.in))) return rc;
    if (rot && rot->out && (rc = subscale_seal_hit(tf, 2, 0, k.tail.seal_out[0] && k.tail.seal_out[1] ? L : 0, p->log_n, k.tail))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    // the checked key switch's own hook, against the call: before anything is launched (keyswitch_checked checks it again)
    if ((rc = ksc_prepare(p))) return rc;
    KscHook h;
    if ((rc = ksc_hook(p, k.form, k.ft, p->acc.as<u64>(), c.d_add0 != nullptr, c.d_add1 != nullptr, h))) return rc;
    k.st = pick(ctx, c.stream);
    // the largest launch's partials (the tail's, [2 L][chunks][2], are fewer than the key's); a rotation keeps sigma(c1)'s seal behind them
    size_t pw = ks_sealed_scratch_words(p);
    if (nb) pw = std::max(pw, ntt_seal_part_words((u32)L, p->log_n, true));
    if (rot) pw = std::max(pw, std::max(galois_seal_part_words((u32)L, p->log_n, true), seal_part_words((u32)L, p->log_n)));
    if ((rc = seal_scratch(ctx, k.st, pw + (rot ? 2 * L : 0), &k.part))) return rc;
    k.behind = k.part + pw;
    k.key.part = k.in.part = k.tail.part = k.part;      // stage 0's verdict is out before stage 3 starts on the same stream, the key's before the tail
    HIP_TRY(hipMemsetAsync(c.d_flags, 0, (size_t)k.lay[nb + 1] * sizeof(u32), k.st));
    return FHE_OK;
}

int ks_sealed_run(const KsSealedCall &c, const KsSealed &k, const uint64_t *d_c, const uint64_t *d_add0)
{
    SealedSteps steps;
    steps.key = &k.key;
    if (c.in_blocks) steps.in = &k.in;
    if (c.rot && c.rot->out) steps.tail = &k.tail;
    return keyswitch_checked(c.p, k.form, c.d_out0, c.d_out1, d_c, c.d_evk, d_add0, c.d_add1, c.a, c.d_flags + k.lay[c.in_blocks + 1], k.st, k.ft, steps);
}
