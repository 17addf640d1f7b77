// mac_sealed.hip -- the two inner products whose long-lived operand is verified on the load that multiplies it (mac_seal.hpp): the
// key switch's, stage 3 of fhe_keyswitch_apply_sealed, fhe_rotate_sealed_fused, fhe_hmult_sealed_fused_key and the sealed hoisted
// rotations, and the BSGS product's inner sum, fhe_bsgs_matvec_sealed.  A translation unit of its own, so that every other kernel
// compiles exactly as before.
//
// k_mac_sealed runs the chunked sweep of seal_sweep.hpp (job loop, workgroup combine, launch) over the family's rows -- the M limb
// rows of the key switch, the limb rows of a giant step -- with the checked kernel's arithmetic (keyswitch_checked.hip,
// bsgs_checked.hip).  Per word: a lane takes two words per step with 16-byte loads of the three operands of every term, digests each
// sealed word from the register it then hands to D::mac, with the weight of its index in the ROW, and stores the two words of each
// half of the sums 16 bytes at a time.  The term loop is inside the element loop and unrolled to T, so a lane's ROWS T SealAcc stay
// in registers.  The job's partial is part[job][slots][2], slots = ROWS terms; a job that saw a sealed word >= q ORs SEAL_RANGE into
// that row's flag, a lane that saw a residue flag ORs it into the [2][rows] words, both with global atomics.  A clean run stores
// nothing beyond the partials.
//
// k_mac_seal_finish, one lane per sealed row slot rows + row: adds the row's partials, makes them canonical and holds them word
// for word against the stored seal; a difference ORs SEAL_SUM.  Without a stored seal it is not launched: the window alone is checked.
//
// Integer arithmetic modulo 2^61 - 1 in the digest: no floating point there, vector stores only.  HOOK: the checked call's
// one-shot fault (BcCheck, the points of residue_check.hpp) and the sealed call's own (KsSealHit, DiagHit: one bit of one sealed
// word in the register as loaded); memory stays clean.
//
// What differs between the families is stated in KsSweep and DiagSweep: the rows and the terms, a row's limb constants, the
// addresses (ntt_launch.hpp, shared with the checked kernels) and the load policy -- the key is read once, so its loads are
// non-temporal as in ks_load_key; the diagonals' keep the default policy, as in k_diag_mac_checked.
//
// Resources, gfx950, from the compiler's resource-usage remarks (-Rpass-analysis=kernel-resource-usage), clean / hooked; scratch
// memory is 0 bytes per lane in every instantiation:
//   key switch, T = 2 / 4 / 8 / 12:  109 / 117, 141 / 149, 235 / 235 VGPRs and 256 VGPRs + 22 / 34 AGPRs; LDS per workgroup 272,
//                                    528, 1040 and 1552 bytes; the compiler's static waves per SIMD 4, 3, 2 and 1
//   BSGS inner sum, T = 4 / 8 / 16:  109 / 118, 142 / 151, 235 / 236 VGPRs; LDS 272, 528 and 1040 bytes; waves per SIMD 4, 3 and 2
// (T = 12, the band of dnum = 9 to 12, keeps its overflow in accumulation registers, not in memory; k_mac_seal_finish: 18 VGPRs).
// What the low occupancy of the wide bands costs on the device: profiles/r26_sealed_mac_fold.md.
#include "bsgs_seal.hpp"
#include "mac_seal.hpp"
#include "seal_sweep.hpp"

namespace fhe {

size_t ks_seal_part_words(u32 M, int logn, u32 dnum) { return ((size_t)M << seal_log_chunks(logn)) * dnum * 4; }
size_t diag_seal_part_words(u32 limbs, int logn, u32 nb) { return ((size_t)limbs << seal_log_chunks(logn)) * nb * 2; }
u32 ks_seal_nd(u32 dnum) { return dnum <= 2 ? 2 : dnum <= 4 ? 4 : dnum <= 8 ? 8 : 12; }
u32 diag_seal_nb(u32 n1) { return n1 <= 4 ? 4 : n1 <= 8 ? 8 : 16; }

namespace {

typedef u64 u64x2 __attribute__((ext_vector_type(2)));

// the key is read once: non-temporal (ks_load_key), two words at a time
__device__ __forceinline__ u64x2 load2_once(const u64 *p) { return __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(p)); }
template <class V> __device__ __forceinline__ void put2(u64 *w, const V &v) { w[0] = v.x, w[1] = v.y; }

} // namespace

// the key switch: row j of M, term d of dnum; KsMacArgs as k_ks_mac_checked takes them with c, ext, evk and acc 16-byte aligned
struct KsSweep : KsSealFamily {
    using Args = KsMacArgs;
    static FHE_HD u32 rows(const Args &a) { return a.M; }
    static FHE_HD u32 terms(const Args &a) { return a.dnum; }
    static __device__ __forceinline__ const LimbParams &limb(const Args &a, u32 j) { return a.lp[j < a.cn ? a.clo + j : j + a.sp_shift]; }
    static __device__ __forceinline__ void load(const Args &a, u32 d, u32 j, u32 i, u64 *x, u64 *k0, u64 *k1)
    {
        ulonglong2 xv;
        const u64 *key = ks_mac_load(a, ks_mac_table_limb(a, j), d, j, i, xv);
        put2(x, xv);
        put2(k0, load2_once(key));
        put2(k1, load2_once(key + ((u64)a.M << a.logn)));
    }
    static __device__ __forceinline__ u64 *out(const Args &a, u32 h, u32 j) { return a.acc + (((u64)h * a.M + j) << a.logn); }
};

// the BSGS inner sum: limb row l of a giant step, term b of n1; DiagMacArgs as k_diag_mac takes them, every buffer 16-byte aligned
struct DiagSweep : DiagSealFamily {
    using Args = DiagMacArgs;
    static FHE_HD u32 rows(const Args &a) { return a.limbs; }
    static FHE_HD u32 terms(const Args &a) { return a.n1; }
    static __device__ __forceinline__ const LimbParams &limb(const Args &a, u32 l) { return a.lp[a.limb0 + l]; }
    static __device__ __forceinline__ void load(const Args &a, u32 b, u32 l, u32 i, u64 *d, u64 *y0, u64 *y1)
    {
        ulonglong2 dv, v0, v1;
        diag_mac_load(a, b, ((u64)l << a.logn) + i, dv, v0, v1);
        put2(d, dv);
        put2(y0, v0);
        put2(y1, v1);
    }
    static __device__ __forceinline__ u64 *out(const Args &a, u32 h, u32 l) { return (h ? a.out1 : a.out0) + ((u64)l << a.logn); }
};

namespace {

// one (row, chunk) job of one arithmetic path: words [i0, i0 + words) of the row
template <class D, class F, int T, bool HOOK>
__device__ __forceinline__ void mac_seal_job(const typename F::Args &a, const BcCheck &k, const MacSealHit &hit, u32 row, u32 i0, u32 words, const LimbParams &p,
                                             SealRows<F::ROWS * T> &g)
{
    const u32 rows = F::rows(a);
    u64 *const out0 = F::out(a, 0, row), *const out1 = F::out(a, 1, row);
    u32 fl0 = 0, fl1 = 0;
    for (u32 t = threadIdx.x * 2; t < words; t += 512) {
        const u32 i = i0 + t;
        const PwFault f0[2] = {fault_at<HOOK>(k, row, i), fault_at<HOOK>(k, row, (u64)i + 1)};
        const PwFault f1[2] = {fault_at<HOOK>(k, rows + row, i), fault_at<HOOK>(k, rows + row, (u64)i + 1)};
        auto ld = [&](u32 term, u64 *u, u64 *v0, u64 *v1) { F::load(a, term, row, i, u, v0, v1); };
        u64 c0[2], c1[2];
        mac_seal_pair<D, F, T, HOOK>(g, F::terms(a), i, p, ld, hit, f0, f1, c0, c1, fl0, fl1);
        *reinterpret_cast<ulonglong2 *>(out0 + i) = ulonglong2{c0[0], c0[1]};
        *reinterpret_cast<ulonglong2 *>(out1 + i) = ulonglong2{c1[0], c1[1]};
    }
    if (fl0) atomicOr(k.flags + row, fl0);
    if (fl1) atomicOr(k.flags + rows + row, fl1);
}

} // namespace

// terms <= T; k.flags = [2][rows] (half, row) as the checked kernel's; part = [rows][chunks][slots][2]; seal_flags = [slots][rows];
// hit = the sealed call's test fault in row hit_row
template <class F, int T, bool HOOK>
__global__ __launch_bounds__(256) void k_mac_sealed(typename F::Args a, BcCheck k, u64 *part, u32 *seal_flags, MacSealHit hit, u32 hit_row)
{
    const u32 rows = F::rows(a), slots = F::ROWS * F::terms(a);
    const SealJobs s(rows, a.logn);
    for (u64 job = blockIdx.x; job < s.jobs; job += gridDim.x) {
        const u32 row = s.unit(job);
        const LimbParams &p = F::limb(a, row);
        MacSealHit h = hit;
        if (HOOK && hit_row != row) h.mask = 0;
        SealRows<F::ROWS * T> g;
        if (p.path == PATH_F64) mac_seal_job<KsDotF64, F, T, HOOK>(a, k, h, row, s.j0(job), s.words, p, g);
        else mac_seal_job<KsDotU64, F, T, HOOK>(a, k, h, row, s.j0(job), s.words, p, g);
        const u32 range = seal_block_combine<true>(g, part + job * 2 * slots, g.range, 2 * slots);      // the rows beyond slots stay unwritten
        if (threadIdx.x == 0) {
            for (u32 r = 0; r < slots; r++)
                if (range >> r & 1) atomicOr(seal_flags + (size_t)r * rows + row, (u32)SEAL_RANGE);
        }
    }
}

// one lane per sealed row r = slot rows + row: seal = [slots rows][2], flags = [slots rows]
__global__ __launch_bounds__(256) void k_mac_seal_finish(const u64 *part, u32 slots, u32 rows, u32 chunks, const u64 *seal, u32 *flags)
{
    const u32 n = slots * rows;
    for (u32 r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        const u32 slot = r / rows, row = r % rows;
        const SealAcc s = seal_merge_partials<SealAcc>(part + ((size_t)row * chunks * slots + slot) * 2, chunks, (size_t)slots * 2);
        if (seal_differs(s.s0, s.s1, seal + 2 * (size_t)r)) atomicOr(flags + r, (u32)SEAL_SUM);
    }
}

namespace {

// the instantiation of band `band`, one of T, More... (the last one where none matches); either hook selects the hooked form
template <class F, int T, int... More>
hipError_t launch_mac_sealed(u32 band, hipStream_t st, const typename F::Args &a, u64 *part, const u64 *seal, u32 *seal_flags, const BcCheck &k,
                             const MacSealHit &hit, u32 hit_row)
{
    if constexpr (sizeof...(More) > 0)
        if (band != (u32)T) return launch_mac_sealed<F, More...>(band, st, a, part, seal, seal_flags, k, hit, hit_row);
    const u32 rows = F::rows(a), slots = F::ROWS * F::terms(a);
    hipError_t e = launch_seal_sweep(k_mac_sealed<F, T, false>, k_mac_sealed<F, T, true>, k.fault_point >= 0 || hit.mask != 0, rows, a.logn, st, a, k, part,
                                     seal_flags, hit, hit_row);
    if (e != hipSuccess || !seal) return e;
    return launch_seal_finish(k_mac_seal_finish, (u64)slots * rows, st, (const u64 *)part, slots, rows, 1u << seal_log_chunks(a.logn), seal, seal_flags);
}

} // namespace

hipError_t launch_ks_mac_sealed(hipStream_t st, const KsMacArgs &a, u64 *part, const u64 *seal_key, u32 *flags_key, const BcCheck &k, const KsSealHit &hit)
{
    if (!a.M || !a.dnum) return hipSuccess;
    if (a.dnum > KS_SEAL_MAX_DNUM || a.logn < 1) return hipErrorInvalidValue;
    return launch_mac_sealed<KsSweep, 2, 4, 8, 12>(ks_seal_nd(a.dnum), st, a, part, seal_key, flags_key, k, MacSealHit{hit.key_row / a.M, hit.coeff, hit.mask},
                                                   hit.key_row % a.M);
}

hipError_t launch_diag_mac_sealed(hipStream_t st, const DiagMacArgs &a, u64 *part, const u64 *seal, u32 *seal_flags, const BcCheck &k, const DiagHit &hit)
{
    if (!a.limbs || !a.n1) return hipSuccess;
    if (a.n1 > DIAG_SEAL_MAX_NB || a.logn < 1) return hipErrorInvalidValue;
    return launch_mac_sealed<DiagSweep, 4, 8, 16>(diag_seal_nb(a.n1), st, a, part, seal, seal_flags, k, MacSealHit{hit.b, hit.coeff, hit.mask}, hit.limb);
}

} // namespace fhe
