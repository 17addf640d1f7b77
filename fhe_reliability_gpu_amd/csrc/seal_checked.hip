// seal_checked.hip -- sealing and verifying rows at rest (seal_check.hpp): fhe_seal, fhe_seal_verify and the sealed composites.
// A translation unit of its own, so that every other kernel compiles exactly as before.
//
// k_row_digest streams the rows once: a row of 2^logn words is cut into chunks of 2^SEAL_LOG_CHUNK words (a whole row below that)
// and the (row, chunk) jobs are spread over the workgroups of a 1-D grid -- operands have few long rows (128 rows of 2^17 words at
// the largest configuration), so one workgroup per row would leave most of the chip idle.  A lane reads 16 bytes per load with
// default cache policy (the sealed calls consume the operand next), adds its two words with the weight of their index in the ROW,
// the 64 lanes of a wave combine by shuffles, the four waves through 64 bytes of LDS, and lane 0 stores the chunk's two partial
// sums.  k_row_digest_finish adds a row's partials in integers modulo p, makes them canonical and either stores the seal or
// compares it with the given one.  Everything is integer arithmetic modulo p, so the seal does not depend on the grid, the chunk
// size or the order of any combination: reruns give identical seals.  No scratch, no floating point, vector stores only.
//
// VERIFY: words are also held against q_l (a violating chunk ORs SEAL_RANGE into its row's flag word with a global atomic; a clean
// run stores nothing extra).  HOOK: the call's one-shot test fault flips one bit of one loaded word in the register, after the load
// and before it is summed or compared: memory stays clean.
#include "checked_kernel.hpp"
#include "seal_check.hpp"

namespace fhe {

size_t seal_part_words(u32 units, int logn) { return ((size_t)units << seal_log_chunks(logn)) * 2; }

// k.flags = [units] (VERIFY only); k.fault_unit = the row, k.fault_coeff = the word; part = [units][chunks][2]
template <bool VERIFY, bool HOOK>
__global__ __launch_bounds__(256) void k_row_digest(SealArgs p, u64 *part, BcCheck k)
{
    __shared__ u64 sh[4][2];
    const int lchunks = seal_log_chunks(p.logn);
    const u32 words = 1u << (p.logn - lchunks);
    const u64 jobs = (u64)p.units << lchunks;
    for (u64 job = blockIdx.x; job < jobs; job += gridDim.x) {
        const u32 unit = (u32)(job >> lchunks), chunk = (u32)(job & (((u64)1 << lchunks) - 1));
        const u32 poly = unit / p.limbs, l = unit % p.limbs;
        const u64 q = p.lp[p.limb0 + l].q;
        const u64 *row = p.x + (((u64)poly * p.poly_stride + l) << p.logn);
        const u32 j0 = chunk * words;
        SealAcc a;
        bool bad = false;
#pragma unroll 4
        for (u32 i = threadIdx.x * 2; i < words; i += 512) {
            const u32 j = j0 + i;
            ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(row + j);
            v.x ^= fault_at<HOOK>(k, unit, j).mask;
            v.y ^= fault_at<HOOK>(k, unit, j + 1).mask;
            a.add(v.x, j);
            a.add(v.y, j + 1);
            if (VERIFY) bad |= v.x >= q || v.y >= q;
        }
        for (int o = 32; o; o >>= 1) a.merge(__shfl_xor(a.s0, o), __shfl_xor(a.s1, o));
        if ((threadIdx.x & 63) == 0) {
            sh[threadIdx.x >> 6][0] = a.s0;
            sh[threadIdx.x >> 6][1] = a.s1;
        }
        const int any_bad = __syncthreads_or(VERIFY && bad);
        if (threadIdx.x == 0) {
            for (int w = 1; w < 4; w++) a.merge(sh[w][0], sh[w][1]);
            part[2 * job] = a.s0;
            part[2 * job + 1] = a.s1;
            if (VERIFY && any_bad) atomicOr(k.flags + unit, (u32)SEAL_RANGE);
        }
        __syncthreads();      // sh is reused by the next job
    }
}

// one lane per row: seal[row] = the canonical sums of its partials, or (VERIFY) flags[row] |= SEAL_SUM where they differ from seal[row]
template <bool VERIFY>
__global__ __launch_bounds__(256) void k_row_digest_finish(const u64 *part, u32 units, u32 chunks, u64 *seal_out, const u64 *seal_in, u32 *flags)
{
    for (u32 u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x) {
        SealAcc a;
        const u64 *pu = part + (size_t)u * chunks * 2;
        for (u32 c = 0; c < chunks; c++) a.merge(pu[2 * c], pu[2 * c + 1]);
        const u64 s0 = seal_canonical(a.s0), s1 = seal_canonical(a.s1);
        if (VERIFY) {
            if (s0 != seal_in[2 * (size_t)u] || s1 != seal_in[2 * (size_t)u + 1]) atomicOr(flags + u, (u32)SEAL_SUM);
        } else {
            seal_out[2 * (size_t)u] = s0;
            seal_out[2 * (size_t)u + 1] = s1;
        }
    }
}

namespace {

// the sweep over (row, chunk) jobs: one workgroup per job up to the cap, a grid-stride loop beyond
dim3 digest_grid(const SealArgs &p) { return dim3(checked_grid(((u64)p.units << seal_log_chunks(p.logn)) * 256, 8192)); }

} // namespace

hipError_t launch_seal(hipStream_t st, const SealArgs &p, u64 *part, u64 *seal, const BcCheck &k)
{
    if (!p.units) return hipSuccess;
    hipError_t e = launch_checked(k_row_digest<false, false>, k_row_digest<false, true>, k, digest_grid(p), st, p, part, k);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_row_digest_finish<false>, dim3(checked_grid(p.units, 1024)), dim3(256), 0, st, (const u64 *)part, p.units,
                       1u << seal_log_chunks(p.logn), seal, (const u64 *)nullptr, (u32 *)nullptr);
    return hipGetLastError();
}

hipError_t launch_seal_verify(hipStream_t st, const SealArgs &p, u64 *part, const u64 *seal, const BcCheck &k)
{
    if (!p.units) return hipSuccess;
    hipError_t e = launch_checked(k_row_digest<true, false>, k_row_digest<true, true>, k, digest_grid(p), st, p, part, k);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_row_digest_finish<true>, dim3(checked_grid(p.units, 1024)), dim3(256), 0, st, (const u64 *)part, p.units,
                       1u << seal_log_chunks(p.logn), (u64 *)nullptr, seal, k.flags);
    return hipGetLastError();
}

} // namespace fhe
