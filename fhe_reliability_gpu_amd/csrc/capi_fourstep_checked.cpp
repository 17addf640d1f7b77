// capi_fourstep_checked.cpp -- the ABFT-checked natural-order (four-step) transform (part of the C ABI of include/fhe_mi355x.h):
// weight tables of a plan, the checksum call that exposes them, and the two checked calls.  The identities and what they do not
// cover: abft_taps.hpp (GsTap); the kernels: fourstep_checked.hip.
#include "capi_internal.hpp"

namespace {

bool capturing(hipStream_t st)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cap);
    return cap != hipStreamCaptureStatusNone;
}

const fhe_ntt_tables *tables_of(const fhe_fourstep *p) { return p->t ? p->t : p->chk->small.get(); }

int zero_weight(const char *table, const std::vector<u64> &w, u64 q)
{
    for (size_t i = 0; i < w.size(); i++)
        if (w[i] % q == 0)
            return fail(FHE_ERR_UNSUPPORTED, std::string("checked four-step: weight table ") + table + " is 0 modulo the modulus at index " + std::to_string(i) +
                                                 " (a fault at that word would be invisible)");
    return FHE_OK;
}

int grow_sums(fhe_fourstep *p, hipStream_t st, size_t n_vec, u32 t1, u32 t2)
{
    fhe_fourstep::Checked &k = *p->chk;
    const size_t need[4] = {n_vec * t1 * 8, n_vec * t1 * 8, n_vec * t2 * 8, n_vec * t2 * 8};
    bool grow = false;
    for (int i = 0; i < 4; i++) grow |= k.sums[i].bytes < need[i];
    if (!grow) return FHE_OK;
    if (capturing(st)) return fail(FHE_ERR_INVALID, "first checked call of this batch size inside a stream capture: run it once outside");
    HIP_TRY(hipStreamSynchronize(st));      // growing frees the old blocks
    for (int i = 0; i < 4; i++) HIP_TRY(k.sums[i].alloc(need[i] * 2));
    return FHE_OK;
}

int prepare(fhe_ctx *ctx, fhe_fourstep *p, hipStream_t st)
{
    if (p->checked_ready) return FHE_OK;
    if (p->big) return fail(FHE_ERR_UNSUPPORTED, "the checked four-step covers plans up to N = 2^20");
    if (capturing(st)) return fail(FHE_ERR_INVALID, "first checked call on this plan inside a stream capture: run fhe_fourstep_prepare_checked once outside");
    const int logn = p->log_n, logp = logn / 2;
    const size_t N = (size_t)1 << logn;
    const u64 q = p->mod;
    std::unique_ptr<fhe_fourstep::Checked> k(new fhe_fourstep::Checked);
    std::vector<u64> v(N), u(N), m;
    for (size_t i = 0; i < N; i++) v[i] = ((i & (((size_t)1 << logp) - 1)) + (i >> logp) + 2) % q;      // generate_weights, negaclic_ntt.py:7-13
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(k->v8.upload(v));
    int rc;
    if (!p->t) {
        // N < 32: u = W v on the host (at most 16 x 16 products), and the modulus' constants for the reduction launches
        const u64 w = host::pow_mod(p->g, (q - 1) / N, q);
        for (size_t kk = 0; kk < N; kk++) {
            const u64 wk = host::pow_mod(w, kk, q);
            u64 acc = 0, cur = 1 % q;
            for (size_t t = 0; t < N; t++) {
                acc = (acc + host::mul_mod(v[t], cur, q)) % q;
                cur = host::mul_mod(cur, wk, q);
            }
            u[kk] = acc;
        }
        std::vector<u64> rows(N);
        host::cyclic_table(q, logn, p->g, false, rows.data());
        fhe_ntt_tables *nt = nullptr;
        if ((rc = build_tables(ctx, logn, &q, 1, rows.data(), false, -1, nullptr, &nt))) return rc;
        k->small.reset(nt);
    } else {
        // u = W^T v = W v: the plan's own unchecked transform, once (fhe_abft_create does the same for w^)
        HIP_TRY(k->u8.alloc(N * 8));
        if ((rc = fhe_fourstep_ntt_batch(ctx, k->u8.as<u64>(), k->v8.as<u64>(), p, 1, st))) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipMemcpy(u.data(), k->u8.p, N * 8, hipMemcpyDeviceToHost));
    }
    if ((rc = zero_weight("v", v, q)) || (rc = zero_weight("u", u, q))) return rc;
    const int path = p->t ? p->t->path[0] : path_for(q);
    if (p->t && logn >= 13) {
        // m = B^T v, B = launch 2's map = the transposed forward column pass: m is the forward column pass of v (the table set's
        // forward slot holds the same cyclic table), which the device's own column pass produces in the arithmetic's lazy form
        DevBuf wb;
        HIP_TRY(wb.upload(v));
        PassArgs pa{wb.as<u64>(), p->t->d_lp.as<LimbParams>(), 0u, 1u, 1u, 1u};
        hipError_t e = launch_ntt(st, pa, logn, false, path, 1, 0);
        if (e != hipSuccess) return hip_fail(e, "launch_ntt(column pass of the weights)");
        HIP_TRY(hipStreamSynchronize(st));
        m.resize(N);
        HIP_TRY(hipMemcpy(m.data(), wb.p, N * 8, hipMemcpyDeviceToHost));
        for (auto &x : m) {
            if (path == PATH_F64) {            // raw FP64 bits of an exact integer in the lazy range
                const long long sv = (long long)u64_bits_to_double(x);
                x = (u64)(((sv % (long long)q) + (long long)q) % (long long)q);
            } else {
                x %= q;                        // [0, 4q)
            }
        }
        if ((rc = zero_weight("m", m, q))) return rc;
    }
    auto enc = [&](const std::vector<u64> &w, DevBuf &plain, DevBuf &tw) -> hipError_t {
        std::vector<Tw> e(w.size());
        for (size_t i = 0; i < w.size(); i++) e[i] = encode(path, w[i], q);
        hipError_t err = plain.upload(w);
        return err != hipSuccess ? err : tw.upload(e);
    };
    HIP_TRY(enc(v, k->v8, k->ev));
    HIP_TRY(enc(u, k->u8, k->eu));
    if (!m.empty()) HIP_TRY(enc(m, k->m8, k->em));
    p->chk = std::move(k);
    u32 t1 = 1, t2 = 1;
    ntt_gs_checked_tiles(logn, &t1, &t2);
    if ((rc = grow_sums(p, st, 16, t1, t2))) {
        p->chk.reset();
        return rc;
    }
    p->checked_ready = true;
    return FHE_OK;
}

// Both checked calls.  The context's two one-shot hooks are read and disarmed first, whatever the outcome.
int fourstep_checked(fhe_ctx *ctx, u64 *d_dst, const u64 *d_src, fhe_fourstep *p, size_t n_vec, uint32_t *d_flags, void *stream, bool phases)
{
    if (!ctx) return fail(FHE_ERR_INVALID, "null argument");
    const long long fidx = ctx->fault_idx;
    const int fbit = ctx->fault_bit, fpass = ctx->pfault_pass;
    ctx->fault_idx = -1;
    ctx->pfault_pass = -1;
    if (!d_dst || !d_src || !p || !d_flags) return fail(FHE_ERR_INVALID, "null argument");
    if (p->big) return fail(FHE_ERR_UNSUPPORTED, "the checked four-step covers plans up to N = 2^20");
    const int logn = p->log_n;
    if (phases && logn < 13)
        return fail(FHE_ERR_UNSUPPORTED, "per-phase checks belong to the two-launch transform (N >= 2^13); single-launch sizes have one phase: use fhe_fourstep_ntt_checked");
    if (fidx >= 0 && logn < 13) return fail(FHE_ERR_UNSUPPORTED, "fault point does not exist at this size: single-launch sizes have no hand-off");
    if (fpass >= 0 && !phases) return fail(FHE_ERR_UNSUPPORTED, "the in-pass fault belongs to fhe_fourstep_ntt_checked_phases");
    if (!n_vec) return FHE_OK;
    if (n_vec > ((size_t)1 << 24)) return fail(FHE_ERR_INVALID, "batch too large for one launch (max 2^24 vectors)");
    const size_t N = (size_t)1 << logn, words = n_vec << logn;
    u32 t1 = 1, t2 = 1;
    ntt_gs_checked_tiles(logn, &t1, &t2);
    if (fidx >= 0 && (u64)fidx >= words) return fail(FHE_ERR_INVALID, "fault index outside the call's window");
    if (fpass >= 0 && ctx->pfault_block >= n_vec * (fpass == 0 ? t1 : t2)) return fail(FHE_ERR_INVALID, "fault workgroup outside the call's launch");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    int rc;
    if ((rc = prepare(ctx, p, st)) || (rc = grow_sums(p, st, n_vec, t1, t2))) return rc;
    fhe_fourstep::Checked &k = *p->chk;
    const LimbParams *lp = tables_of(p)->d_lp.as<LimbParams>();
    u64 *s_in = k.sums[0].as<u64>(), *s_mid1 = k.sums[1].as<u64>(), *s_mid2 = k.sums[2].as<u64>(), *s_out = k.sums[3].as<u64>();
    hipError_t e;
    if (!p->t) {
        // N < 32: separate reduction launches around the unchecked transform (as the checked negacyclic transforms do for tiny sizes)
        if ((e = launch_weighted_checksum(st, s_in, d_src, k.u8.as<u64>(), nullptr, lp, 0u, 1u, (u32)n_vec, 1u, logn)) != hipSuccess) return hip_fail(e, "launch_weighted_checksum");
        if ((rc = fhe_fourstep_ntt_batch(ctx, d_dst, d_src, p, n_vec, st))) return rc;
        if ((e = launch_weighted_checksum(st, s_out, d_dst, k.v8.as<u64>(), nullptr, lp, 0u, 1u, (u32)n_vec, 1u, logn)) != hipSuccess) return hip_fail(e, "launch_weighted_checksum");
        if ((e = launch_compare_flags(st, d_flags, s_in, s_out, (u32)n_vec)) != hipSuccess) return hip_fail(e, "launch_compare_flags");
        return FHE_OK;
    }
    const int path = p->t->path[0];
    const bool two = logn >= 13, hook = fidx >= 0 || fpass >= 0;
    const GsCheckArgs c1{k.eu.as<Tw>(), k.em.as<Tw>(), k.ev.as<Tw>(), k.u8.as<u64>(), k.m8.as<u64>(), logn / 2, s_in, two ? s_mid1 : s_out,
                         fpass, ctx->pfault_block, ctx->pfault_word, ctx->pfault_bit};
    GsCheckArgs c2 = c1;
    c2.sum_a = s_mid2;
    c2.sum_b = s_out;
    // batches that the unchecked call cuts are cut the same way (capi.cpp gs_batch); never with a hook armed.  Sum slots are per vector.
    const size_t per = hook ? 0 : sub_batch_polys(ctx, logn, n_vec, 1);
    bool done = false;
    if (per) {
        if (p->tmp.bytes < words * 8 && capturing(st)) return fail(FHE_ERR_INVALID, "first call of this batch size inside a stream capture: run it once outside");
        u64 *pp = nullptr;
        HIP_TRY(handoff_scratch(ctx, st, per * N * 8, &pp));
        if (pp) {
            rc = for_sub_batches(ctx, st, n_vec, per, per * N * 8, [&](hipStream_t s, size_t p0, size_t cnt, u64 *side_tmp) {
                PassArgs a{d_dst + p0 * N, lp, 0u, 1u, (u32)cnt, 1u};
                a.src = d_src + p0 * N;
                a.stream_hint = ctx->stream_hint != 0;
                GsCheckArgs b1 = c1, b2 = c2;
                b1.sum_a += p0 * t1, b1.sum_b += p0 * t1;
                b2.sum_a += p0 * t2, b2.sum_b += p0 * t2;
                return launch_ntt_gs_checked(s, a, side_tmp ? side_tmp : pp, b1, b2, logn, path, phases, -1);
            });
            if (rc) return rc;
            done = true;
        }
    }
    if (!done) {
        if (two && p->tmp.bytes < words * 8) {
            if (capturing(st)) return fail(FHE_ERR_INVALID, "first call of this batch size inside a stream capture: run it once outside");
            HIP_TRY(hipStreamSynchronize(st));      // growing frees the old block
            HIP_TRY(p->tmp.alloc(words * 8));
        }
        PassArgs a{d_dst, lp, 0u, 1u, (u32)n_vec, 1u};
        a.src = d_src;
        u64 *tmp = p->tmp.as<u64>();
        if (fidx >= 0) {
            // between-launch hook: one bit of one word of the hand-off buffer [n_vec][N]
            if ((e = launch_ntt_gs_checked(st, a, tmp, c1, c2, logn, path, phases, 0)) != hipSuccess) return hip_fail(e, "launch_ntt_gs_checked");
            if ((e = launch_flip_bit(st, tmp, (u64)fidx, fbit)) != hipSuccess) return hip_fail(e, "launch_flip_bit");
            e = launch_ntt_gs_checked(st, a, tmp, c1, c2, logn, path, phases, 1);
        } else {
            e = launch_ntt_gs_checked(st, a, tmp, c1, c2, logn, path, phases, -1);
        }
        if (e != hipSuccess) return hip_fail(e, "launch_ntt_gs_checked");
    }
    if (phases) e = launch_compare_phases(st, d_flags, s_in, s_mid1, t1, s_mid2, s_out, t2, lp, 0u, 1u, (u32)n_vec);
    else e = launch_compare_sums(st, d_flags, s_in, t1, s_out, two ? t2 : t1, lp, 0u, 1u, (u32)n_vec);
    if (e != hipSuccess) return hip_fail(e, "launch_compare");
    return FHE_OK;
}

} // namespace

extern "C" {

int fhe_fourstep_prepare_checked(fhe_ctx *ctx, fhe_fourstep *p, void *stream)
{
    if (!ctx || !p) return fail(FHE_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    return prepare(ctx, p, pick(ctx, stream));
}

int fhe_fourstep_checksum(fhe_ctx *ctx, fhe_fourstep *p, int side, const uint64_t *d_data, uint64_t *d_out, size_t n_vec, void *stream)
{
    if (!ctx || !p || !d_data || !d_out || (side != 0 && side != 1)) return fail(FHE_ERR_INVALID, "bad checksum arguments");
    if (n_vec > ((size_t)1 << 24)) return fail(FHE_ERR_INVALID, "batch too large for one launch (max 2^24 vectors)");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    int rc = prepare(ctx, p, st);
    if (rc) return rc;
    hipError_t e = launch_weighted_checksum(st, d_out, d_data, side ? p->chk->v8.as<u64>() : p->chk->u8.as<u64>(), nullptr, tables_of(p)->d_lp.as<LimbParams>(), 0u, 1u,
                                            (u32)n_vec, 1u, p->log_n);
    if (e != hipSuccess) return hip_fail(e, "launch_weighted_checksum");
    return FHE_OK;
}

int fhe_fourstep_ntt_checked(fhe_ctx *ctx, uint64_t *d_dst, const uint64_t *d_src, fhe_fourstep *p, size_t n_vec, uint32_t *d_flags, void *stream)
{
    return fourstep_checked(ctx, d_dst, d_src, p, n_vec, d_flags, stream, false);
}

int fhe_fourstep_ntt_checked_phases(fhe_ctx *ctx, uint64_t *d_dst, const uint64_t *d_src, fhe_fourstep *p, size_t n_vec, uint32_t *d_flags, void *stream)
{
    return fourstep_checked(ctx, d_dst, d_src, p, n_vec, d_flags, stream, true);
}

} // extern "C"
