// ntt_sealed_io.hpp -- the one kernel behind the sealed forward transform (ntt_fwd_sealed.hip) and the sealed inverse's storing
// launch with an output seal (ntt_inv_sealed_out.hip).  Device code: included by those two translation units only, so that every
// other kernel compiles exactly as before.
//
// k_ntt_pass_sealed_io is k_ntt_pass_abft (ntt_kernels.hip) with SealFwdTap / SealInvTap (ntt_seal_tap.hpp) in place of the ABFT
// tap, in the shape of k_ntt_pass_sealed (ntt_sealed.hip):
//   IN   the launch that loads the transform's input -- every 64-bit word the first register step takes is digested (weight = its
//        index in the row plus one) and held against the window before it is converted; the pass loads from a.src when set;
//   OUT  the launch that stores the result -- every final word is digested on its way to memory with weight = its index in the
//        stored row plus one, next to the ABFT sum over the same word.
// After the phases the workgroup stores its ABFT partials as k_ntt_pass_abft does and combines the lanes' SealAccs and range count
// through wave shuffles and LDS into one integer partial per (row, tile): {S0, S1, n_range} of the input at s.part, {S0, S1} of
// the output at s.part_out -- distinct regions, the single pass writes both.  Integer arithmetic modulo 2^61 - 1 throughout the
// digest, no scratch memory, vector stores only, no atomics.
#pragma once
#include "ntt_launch.hpp"
#include "ntt_plan.hpp"
#include "ntt_seal_tap.hpp"

#include <type_traits>

namespace fhe {

struct SealIoArgs {
    const Tw *win, *wout;
    const u64 *wout8;
    int logp;
    u64 *sum_in, *sum_out;
    u64 *part;            // [rows][tiles][NTT_SEAL_PART], IN
    u64 *part_out;        // [rows][tiles][NTT_SEAL_OUT_PART], OUT (null: the digest is dropped)
    u32 hit_row, hit_coeff;
    u64 hit_mask;
};

// the lanes' sums -> one partial per workgroup at dst (N words, the last COUNTS of them plain counts), through red[waves][N]
template <int N, int COUNTS>
__device__ __forceinline__ void block_seal_store(u64 (&v)[N], u64 (*red)[N], u64 *dst)
{
    for (int o = 32; o; o >>= 1) {
#pragma unroll
        for (int i = 0; i < N; i++) {
            const u64 other = __shfl_xor(v[i], o);
            v[i] = i < N - COUNTS ? seal_fold(v[i] + seal_fold(other)) : v[i] + other;
        }
    }
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) {
#pragma unroll
        for (int i = 0; i < N; i++) red[tid >> 6][i] = v[i];
    }
    __syncthreads();
    if (tid == 0 && dst) {
        for (int w = 1; w < NTT_THREADS / 64; w++) {
#pragma unroll
            for (int i = 0; i < N; i++) v[i] = i < N - COUNTS ? seal_fold(v[i] + seal_fold(red[w][i])) : v[i] + red[w][i];
        }
#pragma unroll
        for (int i = 0; i < N; i++) dst[i] = v[i];
    }
}

// PASS: a column pass (IS_COL) or a row / single pass of the forward (INV = false) or inverse transform.  FP64 instantiations are
// held to four workgroups per CU (128 VGPRs, 4 waves per SIMD, as the unchecked kernels run); the integer path takes what it needs
template <class PASS, int LOGN, bool IS_COL, bool INV, bool IN, bool OUT, bool HOOK>
__global__ __launch_bounds__(NTT_THREADS, PASS::Arith::PATH == PATH_F64 ? 4 : 1) void k_ntt_pass_sealed_io(PassArgs a, SealIoArgs s)
{
    typedef typename PASS::Arith A;
    typedef std::conditional_t<INV, SealInvTap<A, HOOK, IN, OUT>, SealFwdTap<A, HOOK, IN, OUT>> Tap;
    static_assert(IN || !HOOK, "the hook flips a word the launch loads");
    __shared__ __attribute__((aligned(16))) typename PASS::elem lds[PASS::LDS_ELEMS > 0 ? PASS::LDS_ELEMS : 1];
    __shared__ u64 red[2][NTT_THREADS / 64];
    __shared__ u64 sred_in[NTT_THREADS / 64][NTT_SEAL_PART];
    __shared__ u64 sred_out[NTT_THREADS / 64][NTT_SEAL_OUT_PART];
    u32 limb, row0 = 0;
    u64 *base;
    if constexpr (IS_COL) base = col_tile<PASS, LOGN>(blockIdx.x, a, limb);
    else base = row_tile<PASS, LOGN>(blockIdx.x, a, limb, row0);
    // position of the tile inside its limb and index of the row in [poly][limb] order, as k_ntt_pass_abft
    const u32 unit = blockIdx.x / PASS::TILES, tile = blockIdx.x % PASS::TILES, polys = a.units / a.limbs;
    const u32 l = unit / polys, poly = unit % polys, slot = poly * a.poly_stride + l;
    const u32 pos0 = (u32)((base - a.data) & (((size_t)1 << LOGN) - 1));
    const LimbParams &p = a.lp[limb];
    const typename A::Ctx ctx = A::make_ctx(p);
    const TwPtr tw = as_global(INV ? p.inv : p.fwd);
    const Tw inv_n = p.inv_n;
    const int tid = threadIdx.x;
    u32 hit_idx = NTT_SEAL_NO_HIT;
    if constexpr (HOOK) {
        if (slot == s.hit_row) hit_idx = ntt_seal_tile_hit<PASS, IS_COL>(s.hit_coeff, pos0);
    }
    Tap tap{{as_global(s.win) + ((size_t)limb << LOGN) + pos0, as_global(s.wout) + ((size_t)limb << LOGN) + pos0,
             (const u64 FHE_GLOBAL *)s.wout8 + ((size_t)limb << LOGN) + pos0, pos0, s.logp, typename A::elem(0), typename A::elem(0), 0, 0},
            SealAcc{}, 0u, p.q, hit_idx, s.hit_mask, SealAcc{}};
    const u64 *from = IN && a.src ? a.src + (base - a.data) : nullptr;      // out of place: the consuming load reads the sealed rows themselves
    PASS::template phase<0>(tid, base, lds, tw, row0, ctx, inv_n, &tap, from);
    if constexpr (PASS::NPHASE > 1) {
        __syncthreads();
        PASS::template phase<1>(tid, base, lds, tw, row0, ctx, inv_n, &tap);
    }
    if constexpr (PASS::NPHASE > 2) {
        __syncthreads();
        PASS::template phase<2>(tid, base, lds, tw, row0, ctx, inv_n, &tap);
    }
    if constexpr (PASS::NPHASE > 3) {
        __syncthreads();
        PASS::template phase<3>(tid, base, lds, tw, row0, ctx, inv_n, &tap);
    }
    const size_t at = (size_t)slot * PASS::TILES + tile;
    if constexpr (IN) block_sum_mod(A::canonical(tap.acc_in, ctx), p.q, s.sum_in + at, red[0]);
    if constexpr (OUT) block_sum_mod(A::canonical(tap.acc_out, ctx), p.q, s.sum_out + at, red[1]);
    // the tile's digests: lanes -> wave -> workgroup, integers modulo 2^61 - 1 and a plain count
    if constexpr (IN) {
        u64 v[NTT_SEAL_PART] = {tap.seal.s0, tap.seal.s1, tap.n_range};
        block_seal_store<NTT_SEAL_PART, 1>(v, sred_in, s.part + at * NTT_SEAL_PART);
    }
    if constexpr (OUT) {
        u64 v[NTT_SEAL_OUT_PART] = {tap.seal_out.s0, tap.seal_out.s1};
        block_seal_store<NTT_SEAL_OUT_PART, 0>(v, sred_out, s.part_out ? s.part_out + at * NTT_SEAL_OUT_PART : nullptr);
    }
}

template <class PASS, int LOGN, bool IS_COL, bool INV, bool IN, bool OUT>
hipError_t launch_sealed_io(hipStream_t st, const PassArgs &a, const SealIoArgs &s)
{
    const dim3 grid(a.units * PASS::TILES), th(NTT_THREADS);
    if constexpr (IN) {
        if (s.hit_mask) {
            hipLaunchKernelGGL((k_ntt_pass_sealed_io<PASS, LOGN, IS_COL, INV, IN, OUT, true>), grid, th, 0, st, a, s);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((k_ntt_pass_sealed_io<PASS, LOGN, IS_COL, INV, IN, OUT, false>), grid, th, 0, st, a, s);
    return hipGetLastError();
}

} // namespace fhe
