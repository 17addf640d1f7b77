// seal_carry.hip -- the modular add and subtract that carry their operands' seals to the result (seal_carry.hpp): fhe_modadd_sealed,
// fhe_modsub_sealed and the adds of fhe_rotate_sum_sealed.  A translation unit of its own, so that every other kernel compiles
// exactly as before.
//
// k_modadd_carry is k_row_digest (seal_checked.hip) with the operation inside: a row of 2^logn words is cut into chunks of
// 2^SEAL_LOG_CHUNK words and the (row, chunk) jobs are spread over a 1-D grid.  A lane loads 16 bytes of a and of b once, with
// default cache policy (the next sealed call consumes c), forms the two words of c, counts their wraps with the weight of their
// index in the ROW, digests c from the registers it then stores, and the job's sums {s0, s1, [s2], E0, E1, [E2]} combine through
// wave shuffles and 128 or 192 bytes of LDS into one integer partial per job.  A chunk with an operand word >= q ORs SEAL_RANGE
// into its row's flag with a global atomic; a clean run stores nothing extra.  c may be a or b (a lane writes the 16 bytes it read),
// a may be b.
//
// k_modadd_carry_finish, one lane per row: adds the row's partials, predicts the sums of c from the operands' seals (and locators)
// and the wrap sums, ORs SEAL_SUM into the row's flag where digest and prediction differ, and stores the PREDICTED sums, matched
// or not.  The lane reads a row's operand seals before it writes the result's, so d_seal_c may be d_seal_a or d_seal_b.
//
// Integer arithmetic modulo p throughout: no result depends on the grid or on the order of any combination.  No scratch memory,
// no floating point, vector stores only.  HOOK: the one-shot test fault of fhe_ctx_inject_fault_seal_carry, applied in registers
// at one of the five points of seal_carry.hpp; memory stays clean (point 3 is the store itself).
#include "checked_kernel.hpp"
#include "seal_carry.hpp"

namespace fhe {

size_t carry_part_words(u32 units, int logn, bool loc) { return ((size_t)units << seal_log_chunks(logn)) * (loc ? 6 : 4); }

// PointwiseArgs as k_modadd takes them, a / b / c 16-byte aligned and logn >= 1; k.flags = [units]; k.fault_unit = the row,
// k.fault_coeff = the word, k.fault_point = CARRY_AT_*; part = [units][chunks][WORDS]
template <bool SUB, bool LOC, bool HOOK>
__global__ __launch_bounds__(256) void k_modadd_carry(PointwiseArgs p, u64 *part, BcCheck k)
{
    constexpr int W = CarryAcc<LOC>::WORDS;
    __shared__ u64 sh[4][W];
    const int lchunks = seal_log_chunks(p.logn);
    const u32 words = 1u << (p.logn - lchunks);
    const u64 jobs = (u64)p.units << lchunks;
    for (u64 job = blockIdx.x; job < jobs; job += gridDim.x) {
        const u32 unit = (u32)(job >> lchunks), chunk = (u32)(job & (((u64)1 << lchunks) - 1));
        const u32 poly = unit / p.limbs, l = unit % p.limbs;
        const LimbParams &lp = p.lp[p.limb0 + l];
        const u64 q = lp.q, r0 = lp.barrett_lo, r1 = lp.barrett_hi;
        const u64 base = ((u64)poly * p.poly_stride + l) << p.logn;
        const u32 j0 = chunk * words;
        CarryAcc<LOC> acc;
        bool bad = false;
#pragma unroll 4
        for (u32 i = threadIdx.x * 2; i < words; i += 512) {
            const u32 j = j0 + i;
            const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(p.a + base + j);
            const ulonglong2 b = *reinterpret_cast<const ulonglong2 *>(p.b + base + j);
            ulonglong2 c;
            c.x = acc.template step<SUB>(a.x, b.x, q, r0, r1, j, fault_at<HOOK>(k, unit, j), bad);
            c.y = acc.template step<SUB>(a.y, b.y, q, r0, r1, j + 1, fault_at<HOOK>(k, unit, j + 1), bad);
            *reinterpret_cast<ulonglong2 *>(p.c + base + j) = c;
        }
        for (int o = 32; o; o >>= 1) {
            u64 other[W];
#pragma unroll
            for (int i = 0; i < W; i++) other[i] = __shfl_xor(acc.get(i), o);
            acc.merge(other);
        }
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int i = 0; i < W; i++) sh[threadIdx.x >> 6][i] = acc.get(i);
        }
        const int any_bad = __syncthreads_or(bad);
        if (threadIdx.x == 0) {
            for (int w = 1; w < 4; w++) acc.merge(sh[w]);
#pragma unroll
            for (int i = 0; i < W; i++) part[W * job + i] = acc.get(i);
            if (any_bad) atomicOr(k.flags + unit, (u32)SEAL_RANGE);
        }
        __syncthreads();      // sh is reused by the next job
    }
}

// the seals of one carried operation: [units][2] each, and with a locator [units] each
struct CarrySeals {
    const u64 *seal_a, *seal_b, *loc_a, *loc_b;
    u64 *seal_c, *loc_c;
};

// one lane per row (row u on table limb limb0 + u % limbs)
template <bool SUB, bool LOC>
__global__ __launch_bounds__(256) void k_modadd_carry_finish(const u64 *part, u32 units, u32 chunks, const LimbParams *lp, u32 limb0, u32 limbs, CarrySeals s,
                                                             u32 *flags)
{
    constexpr int W = CarryAcc<LOC>::WORDS, S = LOC ? 3 : 2;
    for (u32 u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x) {
        CarryAcc<LOC> acc;
        const u64 *pu = part + (size_t)u * chunks * W;
        for (u32 c = 0; c < chunks; c++) acc.merge(pu + (size_t)c * W);
        u64 got[S], E[S], sa[S], sb[S], pred[S];
#pragma unroll
        for (int i = 0; i < S; i++) got[i] = acc.get(i), E[i] = acc.get(S + i);
        sa[0] = s.seal_a[2 * (size_t)u], sa[1] = s.seal_a[2 * (size_t)u + 1];
        sb[0] = s.seal_b[2 * (size_t)u], sb[1] = s.seal_b[2 * (size_t)u + 1];
        if (LOC) sa[S - 1] = s.loc_a[u], sb[S - 1] = s.loc_b[u];
        if (carry_finish<LOC>(got, E, sa, sb, lp[limb0 + u % limbs].q, SUB, pred)) atomicOr(flags + u, (u32)SEAL_SUM);
        s.seal_c[2 * (size_t)u] = pred[0];
        s.seal_c[2 * (size_t)u + 1] = pred[1];
        if (LOC) s.loc_c[u] = pred[S - 1];
    }
}

namespace {

template <bool SUB, bool LOC>
hipError_t launch_carry(hipStream_t st, const PointwiseArgs &p, u64 *part, const CarrySeals &s, const BcCheck &k)
{
    const u32 chunks = 1u << seal_log_chunks(p.logn);
    hipError_t e = launch_checked(k_modadd_carry<SUB, LOC, false>, k_modadd_carry<SUB, LOC, true>, k, dim3(checked_grid((u64)p.units * chunks * 256, 8192)), st,
                                  p, part, k);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_modadd_carry_finish<SUB, LOC>), dim3(checked_grid(p.units, 1024)), dim3(256), 0, st, (const u64 *)part, p.units, chunks, p.lp, p.limb0,
                       p.limbs, s, k.flags);
    return hipGetLastError();
}

} // namespace

hipError_t launch_modadd_carry(hipStream_t st, const PointwiseArgs &p, bool sub, u64 *part, const u64 *seal_a, const u64 *seal_b, u64 *seal_c,
                               const u64 *loc_a, const u64 *loc_b, u64 *loc_c, const BcCheck &k)
{
    if (!p.units) return hipSuccess;
    const CarrySeals s{seal_a, seal_b, loc_a, loc_b, seal_c, loc_c};
    if (loc_c) return sub ? launch_carry<true, true>(st, p, part, s, k) : launch_carry<false, true>(st, p, part, s, k);
    return sub ? launch_carry<true, false>(st, p, part, s, k) : launch_carry<false, false>(st, p, part, s, k);
}

} // namespace fhe
