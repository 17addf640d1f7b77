// tensor_sealed.hip -- the tensor product with its operands' seals verified on the load that multiplies them and its results
// digested from the registers that are stored (tensor_seal.hpp): fhe_tensor_product_sealed and the tensor step of
// fhe_hmult_sealed_fused.  A translation unit of its own, so that every other kernel compiles exactly as before.
//
// k_tensor_sealed is k_tensor_checked (pointwise_checked.hip) in the shape of k_modadd_carry (seal_carry.hip): a row of 2^logn
// words is cut into chunks of 2^SEAL_LOG_CHUNK words and the (row, chunk) jobs are spread over a 1-D grid.  A lane takes two words
// per step with 16-byte loads of a0, a1, b0, b1, default cache policy (the key switch consumes d2 next), digests each operand word
// from the register it then hands to the product, with the weight of its index in the ROW, forms the two words of d0, d1, d2, with
// OUT digests them as well, and stores them 16 bytes at a time.  After the job the sums combine through wave shuffles and
// 4 x WORDS x 8 bytes of LDS into one integer partial part[job][WORDS]; a lane that saw a residue flag ORs it into the row's
// [3] words, a job that saw an operand word >= q ORs SEAL_RANGE into that operand's row flag, both with global atomics.  A clean
// run stores nothing beyond the partial.  A lane writes only the indices it read, after it read them: an output may be exactly an
// operand's buffer, and a may be b.
//
// k_tensor_seal_finish, one lane per row: adds the row's partials, makes them canonical, holds each operand's pair word for word
// against its stored seal where one was given (a difference ORs SEAL_SUM), and with OUT writes the sums of d0, d1, d2 to the
// output seals that were given.
//
// Integer arithmetic modulo 2^61 - 1 in every digest: no result depends on the grid or on the order of any combination.  No
// scratch memory, vector stores only.  HOOK: the pointwise call's one-shot fault on the d1 sum (BcCheck) and the sealed call's own
// (TensorSealHit: one bit of one operand word in the register as loaded); memory stays clean.
#include "checked_kernel.hpp"
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
    constexpr int W = TensorSealAcc<OUT>::WORDS;
    __shared__ u64 sh[4][W];
    __shared__ u32 shb[4];
    const int lchunks = seal_log_chunks(t.logn);
    const u32 words = 1u << (t.logn - lchunks);
    const u64 jobs = (u64)t.units << lchunks;
    for (u64 job = blockIdx.x; job < jobs; job += gridDim.x) {
        const u32 unit = (u32)(job >> lchunks), chunk = (u32)(job & (((u64)1 << lchunks) - 1));
        TensorSealAcc<OUT> acc;
        u32 bad = 0;
        if (t.lp[t.limb0 + unit % t.limbs].path == PATH_F64) tensor_seal_job<KsDotF64, OUT, HOOK>(t, k, hit, unit, chunk * words, words, acc, bad);
        else tensor_seal_job<KsDotU64, OUT, HOOK>(t, k, hit, unit, chunk * words, words, acc, bad);
        for (int o = 32; o; o >>= 1) {
            u64 other[W];
#pragma unroll
            for (int i = 0; i < W; i++) other[i] = __shfl_xor(acc.get(i), o);
            acc.merge(other);
            bad |= __shfl_xor(bad, o);
        }
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int i = 0; i < W; i++) sh[threadIdx.x >> 6][i] = acc.get(i);
            shb[threadIdx.x >> 6] = bad;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < 4; w++) acc.merge(sh[w]);
#pragma unroll
            for (int i = 0; i < W; i++) part[W * job + i] = acc.get(i);
            bad |= shb[1] | shb[2] | shb[3];
#pragma unroll
            for (int o = 0; o < 4; o++)
                if (bad >> o & 1) atomicOr(t.flags_op[o] + unit, (u32)SEAL_RANGE);
        }
        __syncthreads();      // sh is reused by the next job
    }
}

// one lane per row
template <bool OUT>
__global__ __launch_bounds__(256) void k_tensor_seal_finish(TensorSealArgs t, const u64 *part, u32 chunks)
{
    constexpr int W = TensorSealAcc<OUT>::WORDS;
    for (u32 u = blockIdx.x * blockDim.x + threadIdx.x; u < t.units; u += gridDim.x * blockDim.x) {
        TensorSealAcc<OUT> acc;
        const u64 *pu = part + (size_t)u * chunks * W;
        for (u32 c = 0; c < chunks; c++) acc.merge(pu + (size_t)c * W);
#pragma unroll
        for (int o = 0; o < 4; o++)
            if (t.seal_in[o] && tensor_seal_decide(acc.s[o].s0, acc.s[o].s1, t.seal_in[o] + 2 * (size_t)u)) atomicOr(t.flags_op[o] + u, (u32)SEAL_SUM);
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
    const u32 chunks = 1u << seal_log_chunks(t.logn);
    BcCheck sel = k;      // launch_checked picks the hooked form by the record's point: either hook selects it
    if (hit.mask && sel.fault_point < 0) sel.fault_point = PW_AT_SUM, sel.fault_mask = 0;
    hipError_t e = launch_checked(k_tensor_sealed<OUT, false>, k_tensor_sealed<OUT, true>, sel, dim3(checked_grid((u64)t.units * chunks * 256, TENSOR_SEAL_GRID_CAP)),
                                  st, t, part, sel, hit);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_tensor_seal_finish<OUT>, dim3(checked_grid(t.units, 1024)), dim3(256), 0, st, t, (const u64 *)part, chunks);
    return hipGetLastError();
}

} // namespace

hipError_t launch_tensor_sealed(hipStream_t st, const TensorSealArgs &t, u64 *part, const BcCheck &k, const TensorSealHit &hit)
{
    if (!t.units) return hipSuccess;
    if (t.logn < 1) return hipErrorInvalidValue;
    return t.seal_out[0] || t.seal_out[1] || t.seal_out[2] ? launch_sealed<true>(st, t, part, k, hit) : launch_sealed<false>(st, t, part, k, hit);
}

} // namespace fhe
