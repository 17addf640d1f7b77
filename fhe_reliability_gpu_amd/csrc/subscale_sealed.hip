// subscale_sealed.hip -- the mod-down tail that verifies its first operand on the load that subtracts from it and seals its result
// from the register it stores (subscale_seal.hpp): stage 3 of fhe_rescale_sealed and the last launch of fhe_hmult_sealed_out and
// fhe_rotate_sealed_out.  A translation unit of its own, so that every other kernel compiles exactly as before.
//
// k_sub_scale_sealed runs the chunked sweep of seal_sweep.hpp (job loop, workgroup combine, launch) over the rows (half, limb), with
// k_sub_scale_checked's arithmetic (keyswitch_checked.hip).  Per step a lane takes two adjacent words with 16-byte loads of a, b
// and the addend -- those that exist -- digests the a words from the registers it hands to checked_sub_scale (IN) and the result
// words from the registers it then stores 16 bytes at a time (OUT), each with the weight of its index in the ROW.  The job's
// partial is part[job][2 (IN + OUT)]; lane 0 ORs the job's residue flags into k.flags[half * limbs + limb] and, where an a word
// was >= q, SEAL_RANGE into the row's input flag, both with global atomics.  A clean run stores nothing beyond the partials.
//
// k_sub_scale_seal_finish, one lane per row: adds the row's partials; IN: holds the canonical (S0, S1) of a word for word against
// the stored seal and ORs SEAL_SUM where they differ (a null seal is not compared); OUT: stores the canonical (S0, S1) of the result
// as its seal (a half without a seal buffer is skipped).  Nothing is compared on the output side.
//
// Integer arithmetic modulo 2^61 - 1 in the digest: no floating point, vector stores only, no scratch memory.  HOOK: the checked
// call's one-shot fault (BcCheck, the points of keyswitch_check.hpp) and the sealed tail's own (SubScaleSeal::hit_*: one bit of one
// a word in the register as loaded, or of one result word after its digest); memory stays clean but for that stored word.
// Resources per instantiation: profiles/r21_subscale_sealed.md.
#include "seal_sweep.hpp"
#include "subscale_seal.hpp"

namespace fhe {

size_t subscale_seal_part_words(u32 rows, int logn, bool in) { return ((size_t)rows << seal_log_chunks(logn)) * (in ? 4 : 2); }

// SubScaleArgs as k_sub_scale_checked takes them with every buffer 16-byte aligned and logn >= 1; rows = [halves][limbs], k.flags
// likewise; s as launch_sub_scale_sealed takes it
template <bool IN, bool OUT, bool HOOK>
__global__ __launch_bounds__(256) void k_sub_scale_sealed(SubScaleArgs p, BcCheck k, SubScaleSeal s)
{
    constexpr int W = SubScaleSealAcc<IN, OUT>::WORDS;
    const SealJobs jobs(p.out1 ? 2 * p.limbs : p.limbs, p.logn);
    for (u64 job = blockIdx.x; job < jobs.jobs; job += gridDim.x) {
        const u32 unit = jobs.unit(job), j0 = jobs.j0(job);
        const u32 h = unit / p.limbs, l = unit % p.limbs;
        const LimbParams &lp = p.lp[p.limb0 + l];
        const u64 q = lp.q, r0 = lp.barrett_lo, r1 = lp.barrett_hi, sc = p.scal[l];
        const u32 rq = res64(q);
        const u64 base = (u64)l << p.logn;
        u64 *out = (h ? p.out1 : p.out0) + base;
        const u64 *a = p.a ? p.a + (u64)h * p.a_stride + base : nullptr, *b = p.b ? p.b + (u64)h * p.b_stride + base : nullptr;
        const u64 *add = h ? p.add1 : p.add0;
        if (add) add += base;
        SubScaleSealAcc<IN, OUT> g;
        u32 fl = 0;
#pragma unroll 2
        for (u32 i = threadIdx.x * 2; i < jobs.words; i += 512) {
            const u32 j = j0 + i;
            ulonglong2 av{0, 0}, bv{0, 0}, dv{0, 0};
            if (a) av = *reinterpret_cast<const ulonglong2 *>(a + j);
            if (b) bv = *reinterpret_cast<const ulonglong2 *>(b + j);
            if (add) dv = *reinterpret_cast<const ulonglong2 *>(add + j);
            SubScaleHit h0{-1, 0}, h1{-1, 0};
            if (HOOK && unit == s.hit_row) {
                h0 = SubScaleHit{s.hit_point, j == s.hit_coeff ? s.hit_mask : 0};
                h1 = SubScaleHit{s.hit_point, j + 1 == s.hit_coeff ? s.hit_mask : 0};
            }
            ulonglong2 o;
            o.x = sub_scale_seal_word<IN, OUT, HOOK>(g, SubScaleWord{av.x, bv.x, dv.x, a != nullptr, b != nullptr, add != nullptr}, j, sc, q, r0, r1, rq, fl,
                                                     fault_at<HOOK>(k, unit, j), h0);
            o.y = sub_scale_seal_word<IN, OUT, HOOK>(g, SubScaleWord{av.y, bv.y, dv.y, a != nullptr, b != nullptr, add != nullptr}, j + 1, sc, q, r0, r1, rq, fl,
                                                     fault_at<HOOK>(k, unit, j + 1), h1);
            *reinterpret_cast<ulonglong2 *>(out + j) = o;
        }
        // the residue flags (three bits) and the window bit travel together through the combine
        const u32 m = seal_block_combine<true>(g, s.part + job * W, fl | (g.range ? 0x100u : 0u));
        if (threadIdx.x == 0) {
            if (m & 0xFFu) atomicOr(k.flags + unit, m & 0xFFu);
            if (IN && (m & 0x100u)) atomicOr(s.flags_in + (size_t)h * s.in_stride + l, (u32)SEAL_RANGE);
        }
    }
}

// one lane per row u = (h, l) of the launch
template <bool IN, bool OUT>
__global__ __launch_bounds__(256) void k_sub_scale_seal_finish(const u64 *part, u32 units, u32 limbs, u32 chunks, SubScaleSeal s)
{
    typedef SubScaleSealAcc<IN, OUT> Acc;
    for (u32 u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x) {
        const u32 h = u / limbs, l = u % limbs;
        const Acc g = seal_merge_partials<Acc>(part + (size_t)u * chunks * Acc::WORDS, chunks);
        if (IN) {
            // (the window bit was raised by the sweep itself)
            const size_t r = (size_t)h * s.in_stride + l;
            const u32 v = sub_scale_seal_verdict(g.acc[0].s0, g.acc[0].s1, false, s.seal_in ? s.seal_in + 2 * r : nullptr);
            if (v) atomicOr(s.flags_in + r, v);
        }
        u64 *dst = h ? s.seal_out1 : s.seal_out0;
        if (OUT && dst) {
            const SealAcc &o = g.acc[IN ? 1 : 0];
            dst[2 * (size_t)l] = seal_canonical(o.s0);
            dst[2 * (size_t)l + 1] = seal_canonical(o.s1);
        }
    }
}

namespace {

template <bool IN>
hipError_t launch_sealed(hipStream_t st, const SubScaleArgs &p, const BcCheck &k, const SubScaleSeal &s)
{
    const u32 units = p.out1 ? 2 * p.limbs : p.limbs;
    hipError_t e = launch_seal_sweep(k_sub_scale_sealed<IN, true, false>, k_sub_scale_sealed<IN, true, true>, k.fault_point >= 0 || s.hit_point >= 0, units, p.logn, st,
                                     p, k, s);
    if (e != hipSuccess) return e;
    return launch_seal_finish(k_sub_scale_seal_finish<IN, true>, units, st, (const u64 *)s.part, units, p.limbs, 1u << seal_log_chunks(p.logn), s);
}

} // namespace

hipError_t launch_sub_scale_sealed(hipStream_t st, const SubScaleArgs &p, const BcCheck &k, const SubScaleSeal &s)
{
    if (!p.limbs) return hipSuccess;
    const bool in = s.flags_in != nullptr;
    if (p.logn < 1 || !s.part || !p.out0 || (in && !p.a) || (s.hit_point >= 0 && !sub_scale_seal_point_exists(s.hit_point, in, true))) return hipErrorInvalidValue;
    return in ? launch_sealed<true>(st, p, k, s) : launch_sealed<false>(st, p, k, s);
}

} // namespace fhe
