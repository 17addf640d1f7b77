// tensor_sealed.hip -- the tensor product with its operands' seals verified on the load that multiplies them and its results
// digested from the registers that are stored (tensor_seal.hpp): fhe_tensor_product_sealed and the tensor step of
// fhe_hmult_sealed_fused.  A translation unit of its own, so that every other kernel compiles exactly as before.
//
// k_tensor_sealed runs the chunked sweep of seal_sweep.hpp (job loop, workgroup combine, launch) with k_tensor_checked's
// arithmetic (pointwise_checked.hip).  Per word: a lane takes two words per step with 16-byte loads of a0, a1, b0, b1, default
// cache policy (the key switch consumes d2 next), digests each operand word from the register it then hands to the product, with
// the weight of its index in the ROW, forms the two words of d0, d1, d2, with OUT digests them as well, and stores them 16 bytes
// at a time.  The job's partial is part[job][WORDS] (272 bytes of LDS per workgroup, 464 with OUT); a lane that saw a residue flag
// ORs it into the row's [3] words, a job that saw an operand word >= q ORs SEAL_RANGE into that operand's row flag, both with
// global atomics.  A clean run stores nothing beyond the partial.  A lane writes only the indices it read, after it read them: an
// output may be exactly an operand's buffer, and a may be b.
//
// k_tensor_seal_finish, one lane per row: adds the row's partials, makes them canonical, holds each operand's pair word for word
// against its stored seal where one was given (a difference ORs SEAL_SUM), and with OUT writes the sums of d0, d1, d2 to the
// output seals that were given.
//
// Integer arithmetic modulo 2^61 - 1 in every digest: no result depends on the grid or on the order of any combination.  No
// scratch memory, vector stores only.  HOOK: the pointwise call's one-shot fault on the d1 sum (BcCheck) and the sealed call's own
// (TensorSealHit: one bit of one operand word in the register as loaded); memory stays clean.
#include "seal_sweep.hpp"
#include "tensor_seal.hpp"

namespace fhe {

size_t tensor_seal_part_words(u32 units, int logn, bool out) { return ((size_t)units << seal_log_chunks(logn)) * (out ? 14 : 8); }

// one (row, chunk) job of one arithmetic path: words [j0, j0 + words) of row `unit`
template <class D, bool OUT, bool HOOK>
__device__ __forceinline__ void tensor_seal_job(const TensorSealArgs &t, const BcCheck &k, const TensorSealHit &hit, u32 unit, u32 j0, u32 words,
                                                TensorSealAcc<OUT> &acc, u32 &bad)
{
    const LimbParams &p = t.lp[t.limb0 + unit % t.limbs];
    const u64 base = (u64)unit << t.logn;
    const bool mine = HOOK && hit.mask && hit.row == unit;
    u32 fl[3] = {0, 0, 0};
#pragma unroll 2
    for (u32 i = threadIdx.x * 2; i < words; i += 512) {
        const u32 j = j0 + i;
        const u64 e = base + j;
        const ulonglong2 a0 = *reinterpret_cast<const ulonglong2 *>(t.a0 + e), a1 = *reinterpret_cast<const ulonglong2 *>(t.a1 + e);
        const ulonglong2 b0 = *reinterpret_cast<const ulonglong2 *>(t.b0 + e), b1 = *reinterpret_cast<const ulonglong2 *>(t.b1 + e);
        const u64 x[4] = {a0.x, a1.x, b0.x, b1.x}, y[4] = {a0.y, a1.y, b0.y, b1.y};
        const TensorHit hx{hit.op, mine && hit.coeff == j ? hit.mask : 0}, hy{hit.op, mine && hit.coeff == (u64)j + 1 ? hit.mask : 0};
        u64 dx[3], dy[3];
        u32 fx[3], fy[3];
        acc.template step_on<D>(x, j, p, hx, fault_at<HOOK>(k, unit, j), dx, fx, bad);
        acc.template step_on<D>(y, j + 1, p, hy, fault_at<HOOK>(k, unit, (u64)j + 1), dy, fy, bad);
        *reinterpret_cast<ulonglong2 *>(t.d0 + e) = ulonglong2{dx[0], dy[0]};
        *reinterpret_cast<ulonglong2 *>(t.d1 + e) = ulonglong2{dx[1], dy[1]};
        *reinterpret_cast<ulonglong2 *>(t.d2 + e) = ulonglong2{dx[2], dy[2]};
#pragma unroll
        for (int i3 = 0; i3 < 3; i3++) fl[i3] |= fx[i3] | fy[i3];
    }
#pragma unroll
    for (int i3 = 0; i3 < 3; i3++)
        if (fl[i3]) atomicOr(k.flags + 3 * (u64)unit + i3, fl[i3]);
}

// k.flags = [units][3]; part = [units][chunks][WORDS]
template <bool OUT, bool HOOK>
__global__ __launch_bounds__(256) void k_tensor_sealed(TensorSealArgs t, u64 *part, BcCheck k, TensorSealHit hit)
{
    const SealJobs s(t.units, t.logn);
    for (u64 job = blockIdx.x; job < s.jobs; job += gridDim.x) {
        const u32 unit = s.unit(job);
        TensorSealAcc<OUT> acc;
        u32 bad = 0;
        if (t.lp[t.limb0 + unit % t.limbs].path == PATH_F64) tensor_seal_job<KsDotF64, OUT, HOOK>(t, k, hit, unit, s.j0(job), s.words, acc, bad);
        else tensor_seal_job<KsDotU64, OUT, HOOK>(t, k, hit, unit, s.j0(job), s.words, acc, bad);
        bad = seal_block_combine<true>(acc, part + TensorSealAcc<OUT>::WORDS * job, bad);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int o = 0; o < 4; o++)
                if (bad >> o & 1) atomicOr(t.flags_op[o] + unit, (u32)SEAL_RANGE);
        }
    }
}

// one lane per row
template <bool OUT>
__global__ __launch_bounds__(256) void k_tensor_seal_finish(TensorSealArgs t, const u64 *part, u32 chunks)
{
    constexpr int W = TensorSealAcc<OUT>::WORDS;
    for (u32 u = blockIdx.x * blockDim.x + threadIdx.x; u < t.units; u += gridDim.x * blockDim.x) {
        const TensorSealAcc<OUT> acc = seal_merge_partials<TensorSealAcc<OUT>>(part + (size_t)u * chunks * W, chunks);
#pragma unroll
        for (int o = 0; o < 4; o++)
            if (t.seal_in[o] && seal_differs(acc.s[o].s0, acc.s[o].s1, t.seal_in[o] + 2 * (size_t)u)) atomicOr(t.flags_op[o] + u, (u32)SEAL_SUM);
        if constexpr (OUT) {
#pragma unroll
            for (int i = 0; i < 3; i++)
                if (t.seal_out[i]) {
                    t.seal_out[i][2 * (size_t)u] = seal_canonical(acc.s[TS_D0 + i].s0);
                    t.seal_out[i][2 * (size_t)u + 1] = seal_canonical(acc.s[TS_D0 + i].s1);
                }
        }
    }
}

namespace {

template <bool OUT>
hipError_t launch_sealed(hipStream_t st, const TensorSealArgs &t, u64 *part, const BcCheck &k, const TensorSealHit &hit)
{
    // either hook selects the hooked form
    hipError_t e = launch_seal_sweep(k_tensor_sealed<OUT, false>, k_tensor_sealed<OUT, true>, k.fault_point >= 0 || hit.mask != 0, t.units, t.logn, st, t, part, k, hit);
    if (e != hipSuccess) return e;
    return launch_seal_finish(k_tensor_seal_finish<OUT>, t.units, st, t, (const u64 *)part, 1u << seal_log_chunks(t.logn));
}

} // namespace

hipError_t launch_tensor_sealed(hipStream_t st, const TensorSealArgs &t, u64 *part, const BcCheck &k, const TensorSealHit &hit)
{
    if (!t.units) return hipSuccess;
    if (t.logn < 1) return hipErrorInvalidValue;
    return t.seal_out[0] || t.seal_out[1] || t.seal_out[2] ? launch_sealed<true>(st, t, part, k, hit) : launch_sealed<false>(st, t, part, k, hit);
}

} // namespace fhe
