// bsgs_sealed.hip -- the inner sum of the BSGS product with the diagonals' seals verified on the load that feeds the product
// (bsgs_seal.hpp): fhe_bsgs_matvec_sealed.  A translation unit of its own, so that every other kernel compiles exactly as before.
//
// k_diag_mac_sealed is k_diag_mac_checked (bsgs_checked.hip) in the shape of k_modadd_carry (seal_carry.hip): a limb row of 2^logn
// words is cut into chunks of 2^SEAL_LOG_CHUNK words and the (row, chunk) jobs are spread over a 1-D grid.  A lane takes two words
// per step with 16-byte loads of the diagonal and of both parts of every rotated ciphertext, digests each diagonal word from the
// register it then hands to DiagDot::mac, with the weight of its index in the ROW, and stores the two words of each part.  The b
// loop is inside the element loop and unrolled to NB, so a lane's NB SealAcc stay in registers.  After the job the NB pairs of sums
// combine through wave shuffles and LDS into one integer partial part[job][b][2]; a job that saw a word >= q ORs SEAL_RANGE into
// the (b, l) flag with a global atomic.  A clean run stores nothing beyond the partials.
//
// k_diag_seal_finish, one lane per (b, l): adds the row's partials, makes them canonical and holds them word for word against the
// stored seal; a difference ORs SEAL_SUM.
//
// Integer arithmetic modulo 2^61 - 1 in the digest: no floating point there, no scratch memory, vector stores only.  HOOK: the
// checked call's one-shot fault (BcCheck, the four points of bsgs_check.hpp) and the sealed call's own (DiagHit: one bit of one
// diagonal word in the register as loaded); memory stays clean.
#include "checked_kernel.hpp"
#include "bsgs_seal.hpp"

namespace fhe {

size_t diag_seal_part_words(u32 limbs, int logn, u32 nb) { return ((size_t)limbs << seal_log_chunks(logn)) * nb * 2; }

// one (row, chunk) job of one arithmetic path: words [j0, j0 + words) of limb row l
template <class D, int NB, bool HOOK>
__device__ __forceinline__ void diag_seal_job(const DiagMacArgs &a, const BcCheck &k, const DiagHit &hit, u32 l, u32 j0, u32 words, DiagSeal<NB> &g)
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
    __shared__ u64 sh[4][NB][2];
    __shared__ u32 shr[4];
    const int lchunks = seal_log_chunks(a.logn);
    const u32 words = 1u << (a.logn - lchunks);
    const u32 jobs = a.limbs << lchunks;
    for (u32 job = blockIdx.x; job < jobs; job += gridDim.x) {
        const u32 l = job >> lchunks, chunk = job & ((1u << lchunks) - 1);
        DiagSeal<NB> g;
        if (a.lp[a.limb0 + l].path == PATH_F64) diag_seal_job<KsDotF64, NB, HOOK>(a, k, hit, l, chunk * words, words, g);
        else diag_seal_job<KsDotU64, NB, HOOK>(a, k, hit, l, chunk * words, words, g);
        for (int o = 32; o; o >>= 1) {
            diag_seal_each<0, NB>([&](auto bc) {
                constexpr int b = decltype(bc)::value;
                g.acc[b].merge(__shfl_xor(g.acc[b].s0, o), __shfl_xor(g.acc[b].s1, o));
            });
            g.range |= __shfl_xor(g.range, o);
        }
        if ((threadIdx.x & 63) == 0) {
            diag_seal_each<0, NB>([&](auto bc) {
                constexpr int b = decltype(bc)::value;
                sh[threadIdx.x >> 6][b][0] = g.acc[b].s0;
                sh[threadIdx.x >> 6][b][1] = g.acc[b].s1;
            });
            shr[threadIdx.x >> 6] = g.range;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const u32 range = g.range | shr[1] | shr[2] | shr[3];
            diag_seal_each<0, NB>([&](auto bc) {
                constexpr int b = decltype(bc)::value;
                if ((u32)b < a.n1) {
                    for (int w = 1; w < 4; w++) g.acc[b].merge(sh[w][b][0], sh[w][b][1]);
                    part[((size_t)job * NB + b) * 2] = g.acc[b].s0;
                    part[((size_t)job * NB + b) * 2 + 1] = g.acc[b].s1;
                    if (range >> b & 1) atomicOr(seal_flags + (size_t)b * a.limbs + l, (u32)SEAL_RANGE);
                }
            });
        }
        __syncthreads();      // sh is reused by the next job
    }
}

// one lane per diagonal row u = b * limbs + l of the giant step: seal = [n1 * limbs][2], flags = [n1 * limbs]
__global__ __launch_bounds__(256) void k_diag_seal_finish(const u64 *part, u32 n1, u32 limbs, u32 chunks, u32 nb, const u64 *seal, u32 *flags)
{
    const u32 units = n1 * limbs;
    for (u32 u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x) {
        const u32 b = u / limbs, l = u % limbs;
        SealAcc s;
        for (u32 c = 0; c < chunks; c++) {
            const u64 *pj = part + (((size_t)l * chunks + c) * nb + b) * 2;
            s.merge(pj[0], pj[1]);
        }
        if (diag_seal_decide(s.s0, s.s1, seal + 2 * (size_t)u)) atomicOr(flags + u, (u32)SEAL_SUM);
    }
}

namespace {

template <int NB>
hipError_t launch_sealed(hipStream_t st, const DiagMacArgs &a, u64 *part, const u64 *seal, u32 *seal_flags, const BcCheck &k, const DiagHit &hit)
{
    const u32 chunks = 1u << seal_log_chunks(a.logn);
    const dim3 grid(checked_grid((u64)a.limbs * chunks * 256, 8192));
    hipLaunchKernelGGL((k.fault_point >= 0 || hit.mask ? k_diag_mac_sealed<NB, true> : k_diag_mac_sealed<NB, false>), grid, dim3(256), 0, st, a, k, part, seal_flags,
                       hit);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_diag_seal_finish, dim3(checked_grid((u64)a.n1 * a.limbs, 1024)), dim3(256), 0, st, (const u64 *)part, a.n1, a.limbs, chunks, (u32)NB, seal,
                       seal_flags);
    return hipGetLastError();
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
