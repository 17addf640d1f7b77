// seal_repair.hip -- the locator sum of a sealed row and the repair of one corrupted word per row (seal_check.hpp): fhe_seal_locator,
// fhe_seal_repair and the repairing composites.  A translation unit of its own, so that every other kernel compiles exactly as before.
//
// k_row_locator forms the third sum S2 = sum_j (j + 1)^2 x_j mod p by the chunked sweep of seal_sweep.hpp (job loop, workgroup
// combine, launch).  Per word: 16 bytes per load, the weight of a word its index in the ROW applied twice; one integer partial per
// job, and k_row_locator_finish adds a row's partials and makes the sum canonical.  Integer arithmetic modulo p: the result does
// not depend on the grid or the order of any combination, reruns are identical.
//
// k_row_repair runs after the verifying sweep has filled flags[row]: one workgroup per row, and a workgroup whose row has flag 0
// writes a CLEAN report and moves on -- a clean call costs one nearly empty launch.  For a flagged row the workgroup re-reads the
// whole row and forms S0', S1', S2' afresh (the first sweep's partials are not trusted: its fault may have been in the register),
// counts the words >= q_l and keeps the index of one, lane 0 decides (seal_decide), stores the corrected word, and after a fence
// and a barrier the workgroup sweeps the row a second time: only when all three sums equal the stored ones and every word is in
// its window does the flag drop; otherwise the old word is put back.  No scratch, no floating point, vector stores only.
#include "seal_sweep.hpp"

namespace fhe {

namespace {

// the locator sum alone, at most p + 7 between calls, as the combine of seal_sweep.hpp takes an accumulator
struct LocatorAcc {
    static constexpr int WORDS = 1;
    u64 s2 = 0;
    // folded word f at index j of its row: weight (j + 1)^2
    __device__ void add(u64 f, u32 j) { s2 = seal_fold(s2 + seal_w2mul(f, j + 1)); }
    __device__ u64 get(int) const { return s2; }
    __device__ void merge(const u64 *o) { s2 = seal_fold(s2 + seal_fold(o[0])); }
};

} // namespace

// part = [units][chunks]
__global__ __launch_bounds__(256) void k_row_locator(SealArgs p, u64 *part)
{
    const SealJobs s(p.units, p.logn);
    for (u64 job = blockIdx.x; job < s.jobs; job += gridDim.x) {
        const u32 unit = s.unit(job), j0 = s.j0(job);
        const u32 poly = unit / p.limbs, l = unit % p.limbs;
        const u64 *row = p.x + (((u64)poly * p.poly_stride + l) << p.logn);
        LocatorAcc a;
#pragma unroll 4
        for (u32 i = threadIdx.x * 2; i < s.words; i += 512) {
            const u32 j = j0 + i;
            const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(row + j);
            a.add(seal_fold(v.x), j);
            a.add(seal_fold(v.y), j + 1);
        }
        seal_block_combine<false>(a, part + job);
    }
}

// one lane per row: locator[row] = the canonical sum of its partials
__global__ __launch_bounds__(256) void k_row_locator_finish(const u64 *part, u32 units, u32 chunks, u64 *locator)
{
    for (u32 u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x)
        locator[u] = seal_canonical(seal_merge_partials<LocatorAcc>(part + (size_t)u * chunks, chunks).s2);
}

namespace {

// what a workgroup knows of a row after one sweep, the same in every lane
struct RowSweep {
    u64 got[3];       // canonical S0', S1', S2'
    u32 n_out;        // words >= q
    u32 out_idx;      // the index of one of them (the last), where n_out != 0
};

// all 256 lanes sweep the n words of `row`; sh = [4][5] words of LDS, free again on return
__device__ __forceinline__ RowSweep sweep_row(const u64 *row, u32 n, u64 q, u64 (*sh)[5])
{
    SealAcc3 a;
    u32 n_out = 0, out1 = 0;      // out1 = 1 + the index of a word out of the window
    for (u32 j = threadIdx.x * 2; j < n; j += 512) {
        const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(row + j);
        a.add(v.x, j);
        a.add(v.y, j + 1);
        if (v.x >= q) n_out++, out1 = j + 1;
        if (v.y >= q) n_out++, out1 = j + 2;
    }
    for (int o = 32; o; o >>= 1) {
        a.merge(__shfl_xor(a.s0, o), __shfl_xor(a.s1, o), __shfl_xor(a.s2, o));
        n_out += __shfl_xor(n_out, o);
        const u32 other = __shfl_xor(out1, o);
        out1 = other > out1 ? other : out1;
    }
    if ((threadIdx.x & 63) == 0) {
        u64 *w = sh[threadIdx.x >> 6];
        w[0] = a.s0, w[1] = a.s1, w[2] = a.s2, w[3] = n_out, w[4] = out1;
    }
    __syncthreads();
    SealAcc3 t;
    u32 cnt = 0, idx1 = 0;
    for (int w = 0; w < 4; w++) {
        t.merge(sh[w][0], sh[w][1], sh[w][2]);
        cnt += (u32)sh[w][3];
        idx1 = (u32)sh[w][4] > idx1 ? (u32)sh[w][4] : idx1;
    }
    __syncthreads();      // sh is free again
    return RowSweep{{seal_canonical(t.s0), seal_canonical(t.s1), seal_canonical(t.s2)}, cnt, idx1 ? idx1 - 1 : 0};
}

} // namespace

// flags = [units], filled by the verifying sweep; report = [units][4]
__global__ __launch_bounds__(256) void k_row_repair(SealArgs p, const u64 *seal, const u64 *locator, u32 *flags, u64 *report)
{
    __shared__ u64 sh[4][5];
    __shared__ int verdict;
    const u32 n = 1u << p.logn;
    for (u32 unit = blockIdx.x; unit < p.units; unit += gridDim.x) {
        ulonglong2 *rep = reinterpret_cast<ulonglong2 *>(report + 4 * (size_t)unit);
        if (flags[unit] == 0) {      // the same word in every lane: the branch is uniform
            if (threadIdx.x == 0) rep[0] = make_ulonglong2(SEAL_CLEAN, 0), rep[1] = make_ulonglong2(0, 0);
            continue;
        }
        const u32 poly = unit / p.limbs, l = unit % p.limbs;
        const u64 q = p.lp[p.limb0 + l].q;
        u64 *row = const_cast<u64 *>(p.x) + (((u64)poly * p.poly_stride + l) << p.logn);
        const u64 stored[3] = {seal[2 * (size_t)unit], seal[2 * (size_t)unit + 1], locator[unit]};
        const RowSweep s = sweep_row(row, n, q, sh);
        int status = 0;
        u32 index = 0;
        u64 before = 0, after = 0;
        if (threadIdx.x == 0) {
            const SealVerdict v = seal_decide(s.got, stored, s.n_out, s.out_idx, n);
            status = v.status;
            if (status == SEAL_REPAIRED) {
                index = v.index;      // below n: seal_locate's range, or the index of a word the sweep read
                before = row[index];
                if (seal_repair_word(before, v.d0, q, after)) {
                    row[index] = after;
                    __threadfence();
                } else {
                    status = SEAL_UNCORRECTABLE;
                    index = 0, before = 0, after = 0;
                }
            }
            verdict = status;
        }
        __syncthreads();
        if (verdict == SEAL_REPAIRED) {      // uniform: the confirming sweep, by the whole workgroup
            const RowSweep c = sweep_row(row, n, q, sh);
            if (threadIdx.x == 0 && (c.got[0] != stored[0] || c.got[1] != stored[1] || c.got[2] != stored[2] || c.n_out != 0)) {
                row[index] = before;      // not confirmed: the row is left as it was found
                status = SEAL_UNCORRECTABLE;
                index = 0, before = 0, after = 0;
            }
        }
        if (threadIdx.x == 0) {
            if (status == SEAL_REPAIRED || status == SEAL_TRANSIENT) flags[unit] = 0;
            rep[0] = make_ulonglong2((u64)status, index);
            rep[1] = make_ulonglong2(before, after);
        }
        __syncthreads();      // verdict is reused by the next row
    }
}

hipError_t launch_seal_locator(hipStream_t st, const SealArgs &p, u64 *part, u64 *locator)
{
    if (!p.units) return hipSuccess;
    hipError_t e = launch_seal_sweep(k_row_locator, k_row_locator, false, p.units, p.logn, st, p, part);      // no hooked form
    if (e != hipSuccess) return e;
    return launch_seal_finish(k_row_locator_finish, p.units, st, (const u64 *)part, p.units, 1u << seal_log_chunks(p.logn), locator);
}

hipError_t launch_seal_repair(hipStream_t st, const SealArgs &p, const u64 *seal, const u64 *locator, u32 *flags, u64 *report)
{
    if (!p.units) return hipSuccess;
    hipLaunchKernelGGL(k_row_repair, dim3(checked_grid((u64)p.units * 256, 2048)), dim3(256), 0, st, p, seal, locator, flags, report);
    return hipGetLastError();
}

} // namespace fhe
