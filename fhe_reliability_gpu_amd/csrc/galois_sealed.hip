// galois_sealed.hip -- the NTT-domain Galois permutation with the source's seal verified, and the destination's written, on the
// one gather a permutation makes (galois_seal.hpp): fhe_automorphism_ntt_sealed and the c0 rows of fhe_rotate_hoisted_sealed.  A
// translation unit of its own, so that every other kernel compiles exactly as before.
//
// k_automorphism_ntt_sealed runs the chunked sweep of seal_sweep.hpp (job loop, workgroup combine, launch) over chunks of
// DESTINATION words.  Per word: a lane handles two adjacent destination words per step: two scalar gathers through galois_slot
// (the source words of a chunk lie anywhere in the row), each word digested from the register with its source weight and, with
// OUT, its destination weight, the window counted, and one 16-byte store.  The job's partial is {s0, s1_in, [s1_out], over}: 96 or
// 128 bytes of LDS per workgroup.  The source sums of a row exist only once all its chunks are merged; that merge is why a finish
// launch is needed.
//
// k_galois_seal_finish, one lane per row: adds the row's partials, holds the canonical (s0, s1_in) word for word against
// seal_src[row] (SEAL_SUM), raises SEAL_RANGE where a word was >= q_l, and with OUT stores seal_dst[row] = {the STORED
// seal_src[row][0], canonical s1_out}.  The lane reads the source's seal before it writes, so seal_dst may be seal_src.  The hole
// that is left (galois_seal.hpp): a source change that keeps S0 and moves S1 alone raises the source's flag here and does not poison
// the destination's seal.
//
// Integer arithmetic modulo p throughout: no result depends on the grid or on the order of any combination.  No scratch memory,
// no floating point, vector stores only, no atomics on a clean run.  HOOK: the one-shot test fault of
// fhe_ctx_inject_fault_galois_sealed, applied in registers (GAL_AT_WORD, GAL_AT_INDEX); memory stays clean.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage), clean / hooked: OUT = false 48 / 48 VGPRs and 96 bytes of LDS, OUT =
// true 50 / 48 VGPRs and 128 bytes of LDS; k_galois_seal_finish 20 / 26 VGPRs (OUT = false / true); no scratch memory, no AGPRs and
// 8 waves per SIMD in every instantiation.
#include "galois_seal.hpp"
#include "seal_sweep.hpp"

namespace fhe {

size_t galois_seal_part_words(u32 units, int logn, bool out) { return ((size_t)units << seal_log_chunks(logn)) * (out ? 4 : 3); }

// a.dst / a.src 16-byte aligned and distinct, logn >= 1, k odd; part = [units][chunks][WORDS]; hit.row = the row, hit.coeff = the
// destination word
template <bool OUT, bool HOOK>
__global__ __launch_bounds__(256) void k_automorphism_ntt_sealed(GalSealArgs a, u64 *part, GalSealHit hit)
{
    const SealJobs s(a.units, a.logn);
    for (u64 job = blockIdx.x; job < s.jobs; job += gridDim.x) {
        const u32 unit = s.unit(job), j0 = s.j0(job);
        const u32 poly = unit / a.limbs, l = unit % a.limbs;
        const u64 q = a.lp[a.limb0 + l].q;
        const u64 base = ((u64)poly * a.poly_stride + l) << a.logn;
        const u64 *src_row = a.src + base;
        GalSealAcc<OUT> acc;
#pragma unroll 4
        for (u32 i = threadIdx.x * 2; i < s.words; i += 512) {
            const u32 j = j0 + i;
            const u64 m0 = HOOK && unit == hit.row && j == hit.coeff ? hit.mask : 0, m1 = HOOK && unit == hit.row && j + 1 == hit.coeff ? hit.mask : 0;
            const bool word = !HOOK || hit.point == GAL_AT_WORD;
            ulonglong2 c;
            c.x = galois_seal_step<OUT>(acc, src_row, j, a.logn, a.k, q, word ? m0 : 0, word ? 0u : (u32)m0);
            c.y = galois_seal_step<OUT>(acc, src_row, j + 1, a.logn, a.k, q, word ? m1 : 0, word ? 0u : (u32)m1);
            *reinterpret_cast<ulonglong2 *>(a.dst + base + j) = c;
        }
        seal_block_combine<false>(acc, part + GalSealAcc<OUT>::WORDS * job);      // the window travels as a count, a word of acc
    }
}

// one lane per row; flags zeroed by the caller
template <bool OUT>
__global__ __launch_bounds__(256) void k_galois_seal_finish(const u64 *part, u32 units, u32 chunks, const u64 *seal_src, u64 *seal_dst, u32 *flags)
{
    constexpr int W = GalSealAcc<OUT>::WORDS;
    for (u32 u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x) {
        const GalSealAcc<OUT> acc = seal_merge_partials<GalSealAcc<OUT>>(part + (size_t)u * chunks * W, chunks);
        const u32 f = galois_seal_finish<OUT>(acc, seal_src + 2 * (size_t)u, OUT ? seal_dst + 2 * (size_t)u : nullptr);
        if (f) atomicOr(flags + u, f);
    }
}

namespace {

template <bool OUT>
hipError_t launch_gal_sealed(hipStream_t st, const GalSealArgs &a, u64 *part, const u64 *seal_src, u64 *seal_dst, u32 *flags, const GalSealHit &hit)
{
    hipError_t e = launch_seal_sweep(k_automorphism_ntt_sealed<OUT, false>, k_automorphism_ntt_sealed<OUT, true>, hit.point >= 0, a.units, a.logn, st, a, part, hit);
    if (e != hipSuccess) return e;
    return launch_seal_finish(k_galois_seal_finish<OUT>, a.units, st, (const u64 *)part, a.units, 1u << seal_log_chunks(a.logn), seal_src, seal_dst, flags);
}

} // namespace

hipError_t launch_automorphism_ntt_sealed(hipStream_t st, const GalSealArgs &a, u64 *part, const u64 *seal_src, u64 *seal_dst, u32 *flags,
                                          const GalSealHit &hit)
{
    if (!a.units) return hipSuccess;
    return seal_dst ? launch_gal_sealed<true>(st, a, part, seal_src, seal_dst, flags, hit) : launch_gal_sealed<false>(st, a, part, seal_src, seal_dst, flags, hit);
}

} // namespace fhe
