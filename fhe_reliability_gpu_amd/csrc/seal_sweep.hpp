// seal_sweep.hpp -- the chunked row sweep the seal kernels share (seal_checked.hip, seal_repair.hip, seal_carry.hip,
// galois_sealed.hip, tensor_sealed.hip, subscale_sealed.hip, mac_sealed.hip): the job loop, the workgroup combine, the finish
// kernels' merge and the two launches.  Device side only; the arithmetic of every kernel stays in its own header.
//
// A row of 2^logn words is cut into chunks of 2^SEAL_LOG_CHUNK words (a whole row below that) and the (row, chunk) jobs are spread
// over the workgroups of a 1-D grid, one job per workgroup up to TENSOR_SEAL_GRID_CAP and a grid-stride loop beyond: operands have
// few long rows, so one workgroup per row would leave most of the chip idle.  Inside a job a lane takes two adjacent words per
// step, i = 2 threadIdx.x + 512 t, and accumulates into an accumulator of its kernel's own: anything with a word count WORDS,
// get(i) and merge(const u64 *) (SealAcc, SealRows<N>, CarryAcc, GalSealAcc, TensorSealAcc).  seal_block_combine then makes one
// integer partial of the job, and a finish kernel, one lane per row, adds a row's partials (seal_merge_partials).  The sums are
// integers modulo 2^61 - 1, so no result depends on the grid, the chunking or the order of any combination.
#pragma once
#include "checked_kernel.hpp"
#include "seal_check.hpp"

namespace fhe {

// the (row, chunk) jobs of `units` rows: for (u64 job = blockIdx.x; job < s.jobs; job += gridDim.x).  The counter is 64 bits wide
// everywhere: rows times chunks passes 2^32 long before the words of a batch do
struct SealJobs {
    int lchunks;
    u32 words;      // of one chunk
    u64 jobs;
    __device__ SealJobs(u32 units, int logn) : lchunks(seal_log_chunks(logn)), words(1u << (logn - lchunks)), jobs((u64)units << lchunks) {}
    __device__ u32 unit(u64 job) const { return (u32)(job >> lchunks); }
    // the index in its ROW of the job's first word: the weight of a word is its index in the row, whatever chunk read it
    __device__ u32 j0(u64 job) const { return (u32)(job & (((u64)1 << lchunks) - 1)) * words; }
};

// one step of a wave's butterfly: every lane adds the sums of lane ^ o
template <class Acc> __device__ __forceinline__ void seal_wave_step(Acc &acc, int o)
{
    u64 other[Acc::WORDS];
    seal_each<0, Acc::WORDS>([&](auto ic) { other[decltype(ic)::value] = __shfl_xor(acc.get(decltype(ic)::value), o); });
    acc.merge(other);
}
// the same row by row: with all 2 N words gathered before the first merge the compiler holds k_mac_sealed<KsSweep, 8> and
// k_mac_sealed<DiagSweep, 16> in 249 VGPRs instead of 235, and k_mac_sealed<KsSweep, 12> in 40 AGPRs instead of 22
template <int N> __device__ __forceinline__ void seal_wave_step(SealRows<N> &g, int o)
{
    seal_each<0, N>([&](auto rc) {
        constexpr int r = decltype(rc)::value;
        g.acc[r].merge(__shfl_xor(g.acc[r].s0, o), __shfl_xor(g.acc[r].s1, o));
    });
}

// The one workgroup combine, called by all 256 lanes at the end of a job: the 64 lanes of a wave combine by shuffles, the four
// waves through 4 x WORDS x 8 bytes of LDS, and lane 0 stores the first `store` words of the job's sums to part[0 .. store).  With
// MASK a word of window bits travels along, OR-combined, and is returned to lane 0 (other lanes get a part of it); where the flag
// goes is the kernel's business.  The second barrier is for the next trip of the job loop: a workgroup that has more than one job
// must not write sh before lane 0 has read it.
template <bool MASK, class Acc>
__device__ __forceinline__ u32 seal_block_combine(Acc &acc, u64 *part, u32 mask = 0, u32 store = Acc::WORDS)
{
    constexpr int W = Acc::WORDS;
    __shared__ u64 sh[4][W];
    __shared__ u32 shm[MASK ? 4 : 1];
    for (int o = 32; o; o >>= 1) {
        seal_wave_step(acc, o);
        if (MASK) mask |= __shfl_xor(mask, o);
    }
    if ((threadIdx.x & 63) == 0) {
        seal_each<0, W>([&](auto ic) { sh[threadIdx.x >> 6][decltype(ic)::value] = acc.get(decltype(ic)::value); });
        if (MASK) shm[threadIdx.x >> 6] = mask;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) acc.merge(sh[w]);
        seal_each<0, W>([&](auto ic) {
            if ((u32) decltype(ic)::value < store) part[decltype(ic)::value] = acc.get(decltype(ic)::value);
        });
        if (MASK) mask |= shm[1] | shm[2] | shm[3];
    }
    __syncthreads();      // sh is reused by the next job
    return mask;
}

// a finish kernel's preamble: the sum of a row's `chunks` partials, the first at `part`, one every `stride` words
template <class Acc> __device__ __forceinline__ Acc seal_merge_partials(const u64 *part, u32 chunks, size_t stride = Acc::WORDS)
{
    Acc acc;
    for (u32 c = 0; c < chunks; c++) acc.merge(part + c * stride);
    return acc;
}

// the sweep over the (row, chunk) jobs of `rows` rows: `hooked` when a test fault is armed, `clean` otherwise
template <class... P, class... A>
hipError_t launch_seal_sweep(void (*clean)(P...), void (*hooked)(P...), bool armed, u64 rows, int logn, hipStream_t st, const A &...args)
{
    return launch_armed(clean, hooked, armed, dim3(checked_grid((rows << seal_log_chunks(logn)) * 256, TENSOR_SEAL_GRID_CAP)), st, args...);
}

// the finish kernel over `rows` rows, one lane each
template <class... P, class... A> hipError_t launch_seal_finish(void (*finish)(P...), u64 rows, hipStream_t st, const A &...args)
{
    hipLaunchKernelGGL(finish, dim3(checked_grid(rows, 1024)), dim3(256), 0, st, args...);
    return hipGetLastError();
}

} // namespace fhe
