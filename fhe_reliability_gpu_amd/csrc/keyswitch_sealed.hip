// keyswitch_sealed.hip -- the inner product of the key switch with the key's seals verified on the load that multiplies the key
// (ks_seal.hpp): stage 3 of fhe_keyswitch_apply_sealed, fhe_rotate_sealed_fused and fhe_hmult_sealed_fused_key.  A translation
// unit of its own, so that every other kernel compiles exactly as before.
//
// k_ks_mac_sealed runs the chunked sweep of seal_sweep.hpp (job loop, workgroup combine, launch) over the M rows, with
// k_ks_mac_checked's arithmetic (keyswitch_checked.hip).  Per word: a lane takes two words per step with 16-byte loads of the
// digit (the owned limb of c or its extension) and of both key halves, the key non-temporal as in ks_load_key because it is read
// once, digests each key word from the register it then hands to D::mac, with the weight of its index in the ROW, and stores the
// two words of each half of the sums 16 bytes at a time.  The d loop is inside the element loop and unrolled to ND, so a lane's
// 2 ND SealAcc stay in registers.  The job's partial is part[job][2 dnum][2]; a job that saw a key word >= q ORs SEAL_RANGE into
// that key row's flag, a lane that saw a residue flag ORs it into the [2][M] words, both with global atomics.  A clean run stores
// nothing beyond the partials.
//
// k_ks_seal_finish, one lane per key row r = (d 2 + h) M + j: adds the row's partials, makes them canonical and holds them word for
// word against the stored seal; a difference ORs SEAL_SUM.  Without a stored seal it is not launched: the window alone is checked.
//
// Integer arithmetic modulo 2^61 - 1 in the digest: no floating point there, vector stores only.  HOOK: the checked call's
// one-shot fault (BcCheck, the points of residue_check.hpp) and the sealed call's own (KsSealHit: one bit of one key word in the
// register as loaded); memory stays clean.
//
// Resources, gfx950, from the compiler's resource-usage remarks (-Rpass-analysis=kernel-resource-usage), VGPRs clean / hooked;
// scratch memory is 0 bytes per lane in every instantiation:
//   ND = 2: 108 / 117     ND = 4: 140 / 150     ND = 8: 235 / 236     ND = 12: 256 + 22 AGPRs / 256 + 34 AGPRs
// (ND = 12, the band of dnum = 11, keeps its overflow in accumulation registers, not in memory; k_ks_seal_finish: 18).  LDS per
// workgroup: 272, 528, 1040 and 1552 bytes.  The compiler's static waves per SIMD are 4, 3, 2 and 1; what that costs on the
// device at ND = 8 and 12 is unmeasured.
#include "ks_seal.hpp"
#include "seal_sweep.hpp"

namespace fhe {

size_t ks_seal_part_words(u32 M, int logn, u32 dnum) { return ((size_t)M << seal_log_chunks(logn)) * dnum * 4; }

namespace {

typedef u64 u64x2 __attribute__((ext_vector_type(2)));

// the key is read once: non-temporal (ks_load_key), two words at a time
__device__ __forceinline__ void ks_load_key2(const u64 *p, u64 *k)
{
    const u64x2 v = __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(p));
    k[0] = v.x, k[1] = v.y;
}

// one (row, chunk) job of one arithmetic path: words [i0, i0 + words) of row j
template <class D, int ND, bool HOOK>
__device__ __forceinline__ void ks_seal_job(const KsMacArgs &a, const BcCheck &k, const KsSealHit &hit, u32 j, u32 i0, u32 words, const LimbParams &p,
                                            SealRows<2 * ND> &g)
{
    const u64 N = (u64)1 << a.logn;
    const u32 tl = j < a.cn ? a.clo + j : 0xFFFFFFFFu;     // table limb when the row is a ciphertext limb
    KsHit h{0xFFFFFFFFu, 0, 0, 0};
    if (HOOK && hit.mask && hit.key_row % a.M == j) h = KsHit{hit.key_row / a.M / 2, hit.key_row / a.M % 2, hit.coeff, hit.mask};
    u32 fl0 = 0, fl1 = 0;
    for (u32 t = threadIdx.x * 2; t < words; t += 512) {
        const u32 i = i0 + t;
        const PwFault f0[2] = {fault_at<HOOK>(k, j, i), fault_at<HOOK>(k, j, (u64)i + 1)};
        const PwFault f1[2] = {fault_at<HOOK>(k, a.M + j, i), fault_at<HOOK>(k, a.M + j, (u64)i + 1)};
        auto ld = [&](u32 d, u64 *x, u64 *k0, u64 *k1) {
            const u32 lo = d * a.alpha, hi = lo + a.alpha < a.L ? lo + a.alpha : a.L;
            const u64 *src = (tl >= lo && tl < hi) ? a.c + (u64)j * N + i : a.ext + ((u64)d * a.M + j) * N + i;
            const ulonglong2 xv = *reinterpret_cast<const ulonglong2 *>(src);
            x[0] = xv.x, x[1] = xv.y;
            const u64 *key = a.evk + ((u64)d * 2 * a.M + j) * N + i;
            ks_load_key2(key, k0);
            ks_load_key2(key + (u64)a.M * N, k1);
        };
        u64 c0[2], c1[2];
        ks_seal_pair<D, ND, HOOK>(g, a.dnum, i, p, ld, h, f0, f1, c0, c1, fl0, fl1);
        *reinterpret_cast<ulonglong2 *>(a.acc + (u64)j * N + i) = ulonglong2{c0[0], c0[1]};
        *reinterpret_cast<ulonglong2 *>(a.acc + ((u64)a.M + j) * N + i) = ulonglong2{c1[0], c1[1]};
    }
    if (fl0) atomicOr(k.flags + j, fl0);
    if (fl1) atomicOr(k.flags + a.M + j, fl1);
}

} // namespace

// KsMacArgs as k_ks_mac_checked takes them with c, ext, evk and acc 16-byte aligned, dnum <= ND; k.flags = [2][M] (half, row) as
// k_ks_mac_checked; part = [M][chunks][2 dnum][2]; flags_key = [dnum][2][M]
template <int ND, bool HOOK>
__global__ __launch_bounds__(256) void k_ks_mac_sealed(KsMacArgs a, BcCheck k, u64 *part, u32 *flags_key, KsSealHit hit)
{
    const SealJobs s(a.M, a.logn);
    for (u64 job = blockIdx.x; job < s.jobs; job += gridDim.x) {
        const u32 j = s.unit(job);
        const LimbParams &p = a.lp[j < a.cn ? a.clo + j : j + a.sp_shift];
        SealRows<2 * ND> g;
        if (p.path == PATH_F64) ks_seal_job<KsDotF64, ND, HOOK>(a, k, hit, j, s.j0(job), s.words, p, g);
        else ks_seal_job<KsDotU64, ND, HOOK>(a, k, hit, j, s.j0(job), s.words, p, g);
        const u32 range = seal_block_combine<true>(g, part + job * 4 * a.dnum, g.range, 4 * a.dnum);
        if (threadIdx.x == 0) {
            for (u32 r = 0; r < 2 * a.dnum; r++)      // r = 2 d + h
                if (range >> r & 1) atomicOr(flags_key + (size_t)r * a.M + j, (u32)SEAL_RANGE);
        }
    }
}

// one lane per key row r = (d 2 + h) M + j: seal = [2 dnum M][2], flags = [2 dnum M]
__global__ __launch_bounds__(256) void k_ks_seal_finish(const u64 *part, u32 dnum, u32 M, u32 chunks, const u64 *seal, u32 *flags)
{
    const u32 rows = 2 * dnum * M;
    for (u32 r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += gridDim.x * blockDim.x) {
        const u32 dh = r / M, j = r % M;
        const SealAcc s = seal_merge_partials<SealAcc>(part + ((size_t)j * chunks * 2 * dnum + dh) * 2, chunks, (size_t)dnum * 4);
        if (seal_differs(s.s0, s.s1, seal + 2 * (size_t)r)) atomicOr(flags + r, (u32)SEAL_SUM);
    }
}

namespace {

template <int ND>
hipError_t launch_sealed(hipStream_t st, const KsMacArgs &a, u64 *part, const u64 *seal_key, u32 *flags_key, const BcCheck &k, const KsSealHit &hit)
{
    // either hook selects the hooked form
    hipError_t e = launch_seal_sweep(k_ks_mac_sealed<ND, false>, k_ks_mac_sealed<ND, true>, k.fault_point >= 0 || hit.mask != 0, a.M, a.logn, st, a, k, part,
                                     flags_key, hit);
    if (e != hipSuccess || !seal_key) return e;
    return launch_seal_finish(k_ks_seal_finish, (u64)2 * a.dnum * a.M, st, (const u64 *)part, a.dnum, a.M, 1u << seal_log_chunks(a.logn), seal_key, flags_key);
}

} // namespace

u32 ks_seal_nd(u32 dnum) { return dnum <= 2 ? 2 : dnum <= 4 ? 4 : dnum <= 8 ? 8 : 12; }

hipError_t launch_ks_mac_sealed(hipStream_t st, const KsMacArgs &a, u64 *part, const u64 *seal_key, u32 *flags_key, const BcCheck &k, const KsSealHit &hit)
{
    if (!a.M || !a.dnum) return hipSuccess;
    if (a.dnum > KS_SEAL_MAX_DNUM || a.logn < 1) return hipErrorInvalidValue;
    switch (ks_seal_nd(a.dnum)) {
    case 2: return launch_sealed<2>(st, a, part, seal_key, flags_key, k, hit);
    case 4: return launch_sealed<4>(st, a, part, seal_key, flags_key, k, hit);
    case 8: return launch_sealed<8>(st, a, part, seal_key, flags_key, k, hit);
    default: return launch_sealed<12>(st, a, part, seal_key, flags_key, k, hit);
    }
}

} // namespace fhe
