// bsgs_sealed.hip -- the inner sum of the BSGS product with the diagonals' seals verified on the load that feeds the product
// (bsgs_seal.hpp): fhe_bsgs_matvec_sealed.  A translation unit of its own, so that every other kernel compiles exactly as before.
//
// k_diag_mac_sealed runs the chunked sweep of seal_sweep.hpp (job loop, workgroup combine, launch) over limb rows, with
// k_diag_mac_checked's arithmetic (bsgs_checked.hip).  Per word: a lane takes two words per step with 16-byte loads of the
// diagonal and of both parts of every rotated ciphertext, digests each diagonal word from the register it then hands to
// DiagDot::mac, with the weight of its index in the ROW, and stores the two words of each part.  The b loop is inside the element
// loop and unrolled to NB, so a lane's NB SealAcc stay in registers.  The job's partial is part[job][b][2], b < n1 (LDS per
// workgroup: 272, 528 and 1040 bytes at NB = 4, 8, 16); a job that saw a word >= q ORs SEAL_RANGE into the (b, l) flag with a
// global atomic.  A clean run stores nothing beyond the partials.
//
// k_diag_seal_finish, one lane per (b, l): adds the row's partials, makes them canonical and holds them word for word against the
// stored seal; a difference ORs SEAL_SUM.
//
// Integer arithmetic modulo 2^61 - 1 in the digest: no floating point there, no scratch memory, vector stores only.  HOOK: the
// checked call's one-shot fault (BcCheck, the four points of bsgs_check.hpp) and the sealed call's own (DiagHit: one bit of one
// diagonal word in the register as loaded); memory stays clean.
#include "bsgs_seal.hpp"
#include "seal_sweep.hpp"

namespace fhe {

size_t diag_seal_part_words(u32 limbs, int logn, u32 nb) { return ((size_t)limbs << seal_log_chunks(logn)) * nb * 2; }

// one (row, chunk) job of one arithmetic path: words [j0, j0 + words) of limb row l
template <class D, int NB, bool HOOK>
__device__ __forceinline__ void diag_seal_job(const DiagMacArgs &a, const BcCheck &k, const DiagHit &hit, u32 l, u32 j0, u32 words, SealRows<NB> &g)
{
    const LimbParams &p = a.lp[a.limb0 + l];
    const u64 part = (u64)a.limbs << a.logn;
    const u64 row = (u64)l << a.logn;
    DiagHit h = hit;
    if (HOOK && hit.limb != l) h.mask = 0;
    u32 fl0 = 0, fl1 = 0;
    for (u32 i = threadIdx.x * 2; i < words; i += 512) {
        const u32 j = j0 + i;
        const u64 e = row + j;
        const PwFault f0[2] = {fault_at<HOOK>(k, l, j), fault_at<HOOK>(k, l, (u64)j + 1)};
        const PwFault f1[2] = {fault_at<HOOK>(k, a.limbs + l, j), fault_at<HOOK>(k, a.limbs + l, (u64)j + 1)};
        auto ld = [&](u32 b, u64 *d, u64 *y0, u64 *y1) {
            const ulonglong2 dv = *reinterpret_cast<const ulonglong2 *>(a.diag + (u64)b * part + e);
            const u64 *r = b ? a.rot + (u64)(b - 1) * 2 * part : nullptr;
            const ulonglong2 v0 = *reinterpret_cast<const ulonglong2 *>((b ? r : a.x0) + e);
            const ulonglong2 v1 = *reinterpret_cast<const ulonglong2 *>((b ? r + part : a.x1) + e);
            d[0] = dv.x, d[1] = dv.y;
            y0[0] = v0.x, y0[1] = v0.y;
            y1[0] = v1.x, y1[1] = v1.y;
        };
        u64 c0[2], c1[2];
        diag_seal_pair<D, NB, HOOK>(g, a.n1, j, p, ld, h, f0, f1, c0, c1, fl0, fl1);
        *reinterpret_cast<ulonglong2 *>(a.out0 + e) = ulonglong2{c0[0], c0[1]};
        *reinterpret_cast<ulonglong2 *>(a.out1 + e) = ulonglong2{c1[0], c1[1]};
    }
    if (fl0) atomicOr(k.flags + l, fl0);
    if (fl1) atomicOr(k.flags + a.limbs + l, fl1);
}

// DiagMacArgs as k_diag_mac takes them with every buffer 16-byte aligned, n1 <= NB; k.flags = [2][limbs] (part, limb) as
// k_diag_mac_checked; part = [limbs][chunks][NB][2]; seal_flags = [n1][limbs]
template <int NB, bool HOOK>
__global__ __launch_bounds__(256) void k_diag_mac_sealed(DiagMacArgs a, BcCheck k, u64 *part, u32 *seal_flags, DiagHit hit)
{
    const SealJobs s(a.limbs, a.logn);
    for (u64 job = blockIdx.x; job < s.jobs; job += gridDim.x) {
        const u32 l = s.unit(job);
        SealRows<NB> g;
        if (a.lp[a.limb0 + l].path == PATH_F64) diag_seal_job<KsDotF64, NB, HOOK>(a, k, hit, l, s.j0(job), s.words, g);
        else diag_seal_job<KsDotU64, NB, HOOK>(a, k, hit, l, s.j0(job), s.words, g);
        const u32 range = seal_block_combine<true>(g, part + job * NB * 2, g.range, 2 * a.n1);      // the rows b >= n1 stay unwritten
        if (threadIdx.x == 0) {
            for (u32 b = 0; b < a.n1; b++)
                if (range >> b & 1) atomicOr(seal_flags + (size_t)b * a.limbs + l, (u32)SEAL_RANGE);
        }
    }
}

// one lane per diagonal row u = b * limbs + l of the giant step: seal = [n1 * limbs][2], flags = [n1 * limbs]
__global__ __launch_bounds__(256) void k_diag_seal_finish(const u64 *part, u32 n1, u32 limbs, u32 chunks, u32 nb, const u64 *seal, u32 *flags)
{
    const u32 units = n1 * limbs;
    for (u32 u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x) {
        const u32 b = u / limbs, l = u % limbs;
        const SealAcc s = seal_merge_partials<SealAcc>(part + ((size_t)l * chunks * nb + b) * 2, chunks, (size_t)nb * 2);
        if (seal_differs(s.s0, s.s1, seal + 2 * (size_t)u)) atomicOr(flags + u, (u32)SEAL_SUM);
    }
}

namespace {

template <int NB>
hipError_t launch_sealed(hipStream_t st, const DiagMacArgs &a, u64 *part, const u64 *seal, u32 *seal_flags, const BcCheck &k, const DiagHit &hit)
{
    // either hook selects the hooked form
    hipError_t e = launch_seal_sweep(k_diag_mac_sealed<NB, false>, k_diag_mac_sealed<NB, true>, k.fault_point >= 0 || hit.mask != 0, a.limbs, a.logn, st, a, k, part,
                                     seal_flags, hit);
    if (e != hipSuccess) return e;
    return launch_seal_finish(k_diag_seal_finish, (u64)a.n1 * a.limbs, st, (const u64 *)part, a.n1, a.limbs, 1u << seal_log_chunks(a.logn), (u32)NB, seal, seal_flags);
}

} // namespace

u32 diag_seal_nb(u32 n1) { return n1 <= 4 ? 4 : n1 <= 8 ? 8 : 16; }

hipError_t launch_diag_mac_sealed(hipStream_t st, const DiagMacArgs &a, u64 *part, const u64 *seal, u32 *seal_flags, const BcCheck &k, const DiagHit &hit)
{
    if (!a.limbs || !a.n1) return hipSuccess;
    if (a.n1 > DIAG_SEAL_MAX_NB || a.logn < 1) return hipErrorInvalidValue;
    switch (diag_seal_nb(a.n1)) {
    case 4: return launch_sealed<4>(st, a, part, seal, seal_flags, k, hit);
    case 8: return launch_sealed<8>(st, a, part, seal, seal_flags, k, hit);
    default: return launch_sealed<16>(st, a, part, seal, seal_flags, k, hit);
    }
}

} // namespace fhe
