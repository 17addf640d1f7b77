// galois_checked.hip -- the NTT-domain Galois permutation (aux_kernels.hip k_automorphism_ntt) with one position-weighted sum
// check per unit (galois_check.hpp).  A translation unit of its own, so that the kernels of aux_kernels.hip compile exactly as
// before.  Streams from HBM, one element per lane: the gather through the slot map, the store, and a second linear read of the
// same rows for the source side of the check (an aligned block of 64 slots maps onto an aligned block of 64 slots, so the block
// has just been through the caches).  The residue work is 32-bit lane arithmetic.  A workgroup covers GAL_CHUNK contiguous
// words; at N >= 256 every 256-word step lies in one unit, the lanes keep their partial sums in registers while the unit does
// not change, and the workgroup adds them into the unit's two 64-bit slots with one atomic each (wave shuffle, then four words
// of LDS).  At N < 256 a workgroup's step spans several units: one atomic per lane.
#include "ntt_launch.hpp"
#include "galois_check.hpp"

namespace fhe {

constexpr u32 GAL_THREADS = 256, GAL_STEPS = 8, GAL_CHUNK = GAL_THREADS * GAL_STEPS;

struct GaloisArgs {
    u64 *dst;
    const u64 *src;
    u64 *s_in, *s_out;       // [units] each, zeroed by the launcher's caller
    u32 units;
    int logn;
    u32 k, kinv;
};

// one element: gather, store, both terms.  HOOK: the one-shot test fault is armed (a separate instantiation, so that the clean
// kernel carries no compare against the fault's unit and coefficient)
template <bool HOOK>
__device__ __forceinline__ void galois_element(const GaloisArgs &a, const GaloisFault &f, u64 g, u64 &t_in, u64 &t_out)
{
    const u32 n = 1u << a.logn, j = (u32)g & (n - 1);
    const u64 row = g & ~(u64)(n - 1);
    u64 word_mask = 0;
    u32 index_mask = 0;
    if (HOOK && (u32)(g >> a.logn) == f.unit && j == (u32)f.coeff) {
        if (f.point == GAL_AT_WORD) word_mask = (u64)1 << f.bit;
        else index_mask = 1u << f.bit;
    }
    a.dst[g] = galois_gather(a.src + row, j, a.logn, a.k, word_mask, index_mask, t_out);
    t_in = galois_source_term(a.src[g], j, a.logn, a.kinv);
}

__device__ __forceinline__ u64 gal_wave_sum(u64 v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

template <bool HOOK>
__global__ __launch_bounds__(GAL_THREADS) void k_automorphism_ntt_checked(GaloisArgs a, GaloisFault f)
{
    __shared__ u64 red[2][GAL_THREADS / 64];
    const u64 total = (u64)a.units << a.logn;
    const u64 base = blockIdx.x * (u64)GAL_CHUNK;
    if (a.logn < 8) {
        for (u32 s = 0; s < GAL_STEPS; s++) {
            const u64 g = base + (u64)s * GAL_THREADS + threadIdx.x;
            if (g >= total) return;
            u64 t_in, t_out;
            galois_element<HOOK>(a, f, g, t_in, t_out);
            const u32 unit = (u32)(g >> a.logn);
            atomicAdd((unsigned long long *)a.s_in + unit, (unsigned long long)t_in);
            atomicAdd((unsigned long long *)a.s_out + unit, (unsigned long long)t_out);
        }
        return;
    }
    // N >= 256: total is a multiple of 256, so every step is whole and its unit is the same for the whole workgroup
    u64 acc_in = 0, acc_out = 0;
    u32 cur = (u32)(base >> a.logn);
    auto flush = [&](u32 unit) {
        const u64 w_in = gal_wave_sum(acc_in), w_out = gal_wave_sum(acc_out);
        if ((threadIdx.x & 63) == 0) {
            red[0][threadIdx.x >> 6] = w_in;
            red[1][threadIdx.x >> 6] = w_out;
        }
        __syncthreads();
        if (threadIdx.x < 2) {
            u64 s = 0;
            for (u32 w = 0; w < GAL_THREADS / 64; w++) s += red[threadIdx.x][w];
            atomicAdd((unsigned long long *)(threadIdx.x ? a.s_out : a.s_in) + unit, (unsigned long long)s);
        }
        __syncthreads();
        acc_in = acc_out = 0;
    };
    for (u32 s = 0; s < GAL_STEPS; s++) {
        const u64 g0 = base + (u64)s * GAL_THREADS;
        if (g0 >= total) break;
        const u32 unit = (u32)(g0 >> a.logn);
        if (unit != cur) {
            flush(cur);
            cur = unit;
        }
        u64 t_in, t_out;
        galois_element<HOOK>(a, f, g0 + threadIdx.x, t_in, t_out);
        acc_in += t_in;
        acc_out += t_out;
    }
    flush(cur);
}

__global__ void k_galois_compare(u32 *flags, const u64 *s_in, const u64 *s_out, u32 units)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < units) flags[i] = galois_sums_flag(s_in[i], s_out[i]);
}

hipError_t launch_automorphism_ntt_checked(hipStream_t st, u64 *dst, const u64 *src, u64 *s_in, u64 *s_out, u32 units, int logn, u32 k, u32 kinv,
                                           const GaloisFault &f)
{
    const u64 total = (u64)units << logn;
    if (!total) return hipSuccess;
    const u64 blocks = (total + GAL_CHUNK - 1) / GAL_CHUNK;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const GaloisArgs a{dst, src, s_in, s_out, units, logn, k, kinv};
    if (f.point >= 0) hipLaunchKernelGGL(k_automorphism_ntt_checked<true>, dim3((u32)blocks), dim3(GAL_THREADS), 0, st, a, f);
    else hipLaunchKernelGGL(k_automorphism_ntt_checked<false>, dim3((u32)blocks), dim3(GAL_THREADS), 0, st, a, f);
    return hipGetLastError();
}

hipError_t launch_galois_compare(hipStream_t st, u32 *flags, const u64 *s_in, const u64 *s_out, u32 units)
{
    if (!units) return hipSuccess;
    hipLaunchKernelGGL(k_galois_compare, dim3((units + 255) / 256), dim3(256), 0, st, flags, s_in, s_out, units);
    return hipGetLastError();
}

} // namespace fhe
