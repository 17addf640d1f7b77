// seal_carry.hip -- the modular add and subtract that carry their operands' seals to the result (seal_carry.hpp): fhe_modadd_sealed,
// fhe_modsub_sealed and the adds of fhe_rotate_sum_sealed.  A translation unit of its own, so that every other kernel compiles
// exactly as before.
//
// k_modadd_carry runs the chunked sweep of seal_sweep.hpp (job loop, workgroup combine, launch).  Per word: a lane loads 16 bytes
// of a and of b once, with default cache policy (the next sealed call consumes c), forms the two words of c, counts their wraps
// with the weight of their index in the ROW and digests c from the registers it then stores; the job's partial is {s0, s1, [s2],
// E0, E1, [E2]}.  LDS per workgroup, from the compiler: 144 bytes, 208 with a locator (the sums of four waves and their window
// bits).  A chunk with an operand word >= q ORs SEAL_RANGE into its row's flag with a global atomic; a clean run stores nothing
// extra.  c may be a or b (a lane writes the 16 bytes it read), a may be b.
//
// k_modadd_carry_finish, one lane per row: adds the row's partials, predicts the sums of c from the operands' seals (and locators)
// and the wrap sums, ORs SEAL_SUM into the row's flag where digest and prediction differ, and stores the PREDICTED sums, matched
// or not.  The lane reads a row's operand seals before it writes the result's, so d_seal_c may be d_seal_a or d_seal_b.
//
// Integer arithmetic modulo p throughout: no result depends on the grid or on the order of any combination.  No scratch memory,
// no floating point, vector stores only.  HOOK: the one-shot test fault of fhe_ctx_inject_fault_seal_carry, applied in registers
// at one of the five points of seal_carry.hpp; memory stays clean (point 3 is the store itself).
#include "seal_carry.hpp"
#include "seal_sweep.hpp"

namespace fhe {

size_t carry_part_words(u32 units, int logn, bool loc) { return ((size_t)units << seal_log_chunks(logn)) * (loc ? 6 : 4); }

// PointwiseArgs as k_modadd takes them, a / b / c 16-byte aligned and logn >= 1; k.flags = [units]; k.fault_unit = the row,
// k.fault_coeff = the word, k.fault_point = CARRY_AT_*; part = [units][chunks][WORDS]
template <bool SUB, bool LOC, bool HOOK>
__global__ __launch_bounds__(256) void k_modadd_carry(PointwiseArgs p, u64 *part, BcCheck k)
{
    const SealJobs s(p.units, p.logn);
    for (u64 job = blockIdx.x; job < s.jobs; job += gridDim.x) {
        const u32 unit = s.unit(job), j0 = s.j0(job);
        const u32 poly = unit / p.limbs, l = unit % p.limbs;
        const LimbParams &lp = p.lp[p.limb0 + l];
        const u64 q = lp.q, r0 = lp.barrett_lo, r1 = lp.barrett_hi;
        const u64 base = ((u64)poly * p.poly_stride + l) << p.logn;
        CarryAcc<LOC> acc;
        bool bad = false;
#pragma unroll 4
        for (u32 i = threadIdx.x * 2; i < s.words; i += 512) {
            const u32 j = j0 + i;
            const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(p.a + base + j);
            const ulonglong2 b = *reinterpret_cast<const ulonglong2 *>(p.b + base + j);
            ulonglong2 c;
            c.x = acc.template step<SUB>(a.x, b.x, q, r0, r1, j, fault_at<HOOK>(k, unit, j), bad);
            c.y = acc.template step<SUB>(a.y, b.y, q, r0, r1, j + 1, fault_at<HOOK>(k, unit, j + 1), bad);
            *reinterpret_cast<ulonglong2 *>(p.c + base + j) = c;
        }
        const u32 any_bad = seal_block_combine<true>(acc, part + CarryAcc<LOC>::WORDS * job, bad);
        if (threadIdx.x == 0 && any_bad) atomicOr(k.flags + unit, (u32)SEAL_RANGE);
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
        const CarryAcc<LOC> acc = seal_merge_partials<CarryAcc<LOC>>(part + (size_t)u * chunks * W, chunks);
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
    hipError_t e = launch_seal_sweep(k_modadd_carry<SUB, LOC, false>, k_modadd_carry<SUB, LOC, true>, k.fault_point >= 0, p.units, p.logn, st, p, part, k);
    if (e != hipSuccess) return e;
    return launch_seal_finish(k_modadd_carry_finish<SUB, LOC>, p.units, st, (const u64 *)part, p.units, 1u << seal_log_chunks(p.logn), p.lp, p.limb0, p.limbs, s,
                              k.flags);
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
