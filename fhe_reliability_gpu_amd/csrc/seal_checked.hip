// seal_checked.hip -- sealing and verifying rows at rest (seal_check.hpp): fhe_seal, fhe_seal_verify and the sealed composites.
// A translation unit of its own, so that every other kernel compiles exactly as before.
//
// k_row_digest streams the rows once, by the chunked sweep of seal_sweep.hpp (job loop, workgroup combine, launch).  Per word: a
// lane reads 16 bytes per load with default cache policy (the sealed calls consume the operand next) and adds its two words with
// the weight of their index in the ROW; the job's partial is the chunk's two sums.  k_row_digest_finish adds a row's partials in
// integers modulo p, makes them canonical and either stores the seal or compares it with the given one.  Everything is integer
// arithmetic modulo p, so the seal does not depend on the grid, the chunk size or the order of any combination: reruns give
// identical seals.  No scratch, no floating point, vector stores only.
//
// VERIFY: words are also held against q_l (a violating chunk ORs SEAL_RANGE into its row's flag word with a global atomic; a clean
// run stores nothing extra).  HOOK: the call's one-shot test fault flips one bit of one loaded word in the register, after the load
// and before it is summed or compared: memory stays clean.
#include "seal_sweep.hpp"

namespace fhe {

size_t seal_part_words(u32 units, int logn) { return ((size_t)units << seal_log_chunks(logn)) * 2; }

// k.flags = [units] (VERIFY only); k.fault_unit = the row, k.fault_coeff = the word; part = [units][chunks][2]
template <bool VERIFY, bool HOOK>
__global__ __launch_bounds__(256) void k_row_digest(SealArgs p, u64 *part, BcCheck k)
{
    const SealJobs s(p.units, p.logn);
    for (u64 job = blockIdx.x; job < s.jobs; job += gridDim.x) {
        const u32 unit = s.unit(job), j0 = s.j0(job);
        const u32 poly = unit / p.limbs, l = unit % p.limbs;
        const u64 q = p.lp[p.limb0 + l].q;
        const u64 *row = p.x + (((u64)poly * p.poly_stride + l) << p.logn);
        SealAcc a;
        bool bad = false;
#pragma unroll 4
        for (u32 i = threadIdx.x * 2; i < s.words; i += 512) {
            const u32 j = j0 + i;
            ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(row + j);
            v.x ^= fault_at<HOOK>(k, unit, j).mask;
            v.y ^= fault_at<HOOK>(k, unit, j + 1).mask;
            a.add(v.x, j);
            a.add(v.y, j + 1);
            if (VERIFY) bad |= v.x >= q || v.y >= q;
        }
        const u32 any_bad = seal_block_combine<VERIFY>(a, part + 2 * job, bad);
        if (VERIFY && threadIdx.x == 0 && any_bad) atomicOr(k.flags + unit, (u32)SEAL_RANGE);
    }
}

// one lane per row: seal[row] = the canonical sums of its partials, or (VERIFY) flags[row] |= SEAL_SUM where they differ from seal[row]
template <bool VERIFY>
__global__ __launch_bounds__(256) void k_row_digest_finish(const u64 *part, u32 units, u32 chunks, u64 *seal_out, const u64 *seal_in, u32 *flags)
{
    for (u32 u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x) {
        const SealAcc a = seal_merge_partials<SealAcc>(part + (size_t)u * chunks * 2, chunks);
        if (VERIFY) {
            if (seal_differs(a.s0, a.s1, seal_in + 2 * (size_t)u)) atomicOr(flags + u, (u32)SEAL_SUM);
        } else {
            seal_out[2 * (size_t)u] = seal_canonical(a.s0);
            seal_out[2 * (size_t)u + 1] = seal_canonical(a.s1);
        }
    }
}

hipError_t launch_seal(hipStream_t st, const SealArgs &p, u64 *part, u64 *seal, const BcCheck &k)
{
    if (!p.units) return hipSuccess;
    hipError_t e = launch_seal_sweep(k_row_digest<false, false>, k_row_digest<false, true>, k.fault_point >= 0, p.units, p.logn, st, p, part, k);
    if (e != hipSuccess) return e;
    return launch_seal_finish(k_row_digest_finish<false>, p.units, st, (const u64 *)part, p.units, 1u << seal_log_chunks(p.logn), seal, (const u64 *)nullptr,
                              (u32 *)nullptr);
}

hipError_t launch_seal_verify(hipStream_t st, const SealArgs &p, u64 *part, const u64 *seal, const BcCheck &k)
{
    if (!p.units) return hipSuccess;
    hipError_t e = launch_seal_sweep(k_row_digest<true, false>, k_row_digest<true, true>, k.fault_point >= 0, p.units, p.logn, st, p, part, k);
    if (e != hipSuccess) return e;
    return launch_seal_finish(k_row_digest_finish<true>, p.units, st, (const u64 *)part, p.units, 1u << seal_log_chunks(p.logn), (u64 *)nullptr, seal, k.flags);
}

} // namespace fhe
