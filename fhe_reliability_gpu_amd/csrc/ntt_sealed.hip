// ntt_sealed.hip -- the sealed transforms' public launcher, the inverse direction's kernels and the two finish kernels
// (ntt_seal_tap.hpp, ntt_sealed_io.hpp): fhe_ntt_inverse_sealed, fhe_ntt_inverse_sealed_out, stage 0 of
// fhe_keyswitch_apply_sealed_in / fhe_rotate_sealed_in.  The forward direction's kernels compile in ntt_fwd_sealed.hip.
//
// k_ntt_seal_finish, one lane per row: merges the tiles' input partials, holds the canonical (S0, S1) word for word against
// seal_src[row] (SEAL_SUM; a null seal pointer is not compared), raises SEAL_RANGE where a word was >= q_l, and stores the row's
// flag word.
//
// k_ntt_seal_out_finish, one lane per row, runs after launch_compare_sums: it merges the row's output partials and writes
// seal_dst[row] by the poison rule (ntt_seal_tap.hpp ntt_seal_out) -- the canonical pair where the row's input verdict and its
// ABFT flag are both zero, {~0, ~0} otherwise.  A ROW WITH ANY RAISED FLAG LEAVES THE CALL WITH A SEAL THAT CAN NEVER VERIFY.
#include "ntt_sealed_io.hpp"

namespace fhe {

// one lane per row of the launch: row u = (poly, l) at slot poly * poly_stride + l; every row's flag word is written
__global__ __launch_bounds__(256) void k_ntt_seal_finish(const u64 *part, u32 tiles, u32 units, u32 limbs, u32 poly_stride, const u64 *seal_src, u32 *flags)
{
    for (u32 u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x) {
        const u32 slot = (u / limbs) * poly_stride + u % limbs;
        const u64 *pu = part + (size_t)slot * tiles * NTT_SEAL_PART;
        SealAcc acc;
        u64 nr = 0;
        for (u32 t = 0; t < tiles; t++) {
            acc.merge(pu[(size_t)t * NTT_SEAL_PART], pu[(size_t)t * NTT_SEAL_PART + 1]);
            nr += pu[(size_t)t * NTT_SEAL_PART + 2];
        }
        flags[slot] = ntt_seal_verdict(acc, nr, seal_src ? seal_src + 2 * (size_t)slot : nullptr);
    }
}

hipError_t launch_ntt_seal_finish(hipStream_t st, const PassArgs &a, u32 tiles, const NttSealIn &s)
{
    const u32 fgrid = (a.units + 255) / 256;
    hipLaunchKernelGGL(k_ntt_seal_finish, dim3(fgrid < 1024 ? fgrid : 1024), dim3(256), 0, st, (const u64 *)s.part, tiles, a.units, a.limbs, a.poly_stride, s.seal_src,
                       s.flags);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_ntt_seal_out_finish(const u64 *part_out, u32 tiles, u32 rows, const u32 *flags_in, const u32 *flags_in2, const u32 *flags_abft,
                                                             u32 abft_words, u64 *seal_dst)
{
    for (u32 r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += gridDim.x * blockDim.x) {
        const u64 *pr = part_out + (size_t)r * tiles * NTT_SEAL_OUT_PART;
        SealAcc acc;
        for (u32 t = 0; t < tiles; t++) acc.merge(pr[(size_t)t * NTT_SEAL_OUT_PART], pr[(size_t)t * NTT_SEAL_OUT_PART + 1]);
        u32 fin = flags_in[r] | (flags_in2 ? flags_in2[r] : 0u), fab = 0;
        for (u32 w = 0; w < abft_words; w++) fab |= flags_abft[(size_t)r * abft_words + w];
        u64 out[2];
        ntt_seal_out(acc, fin, fab, out);
        seal_dst[2 * (size_t)r] = out[0];
        seal_dst[2 * (size_t)r + 1] = out[1];
    }
}

hipError_t launch_ntt_seal_out_finish(hipStream_t st, const u64 *part_out, u32 tiles, u32 rows, const u32 *flags_in, const u32 *flags_abft, u64 *seal_dst,
                                      const u32 *flags_in2, u32 abft_words)
{
    if (!rows) return hipSuccess;
    const u32 grid = (rows + 255) / 256;
    hipLaunchKernelGGL(k_ntt_seal_out_finish, dim3(grid < 1024 ? grid : 1024), dim3(256), 0, st, part_out, tiles, rows, flags_in, flags_in2, flags_abft, abft_words,
                       seal_dst);
    return hipGetLastError();
}

size_t ntt_seal_part_words(u32 rows, int logn, bool inverse)
{
    u32 tin = 1, tout = 1;
    ntt_checked_tiles(logn, &tin, &tout, inverse);
    return (size_t)rows * tin * NTT_SEAL_PART;
}

size_t ntt_seal_out_part_words(u32 rows, int logn, bool inverse)
{
    u32 tin = 1, tout = 1;
    ntt_checked_tiles(logn, &tin, &tout, inverse);
    return (size_t)rows * tout * NTT_SEAL_OUT_PART;
}

template hipError_t launch_ntt_sealed_dir<true>(hipStream_t, const PassArgs &, const SealIoArgs &, int, int, int, const NttSealIn &);

hipError_t launch_ntt_sealed(hipStream_t st, const PassArgs &a, const Tw *win, const Tw *wout, const u64 *wout8, u64 *sum_in, u64 *sum_out, int logn, int path,
                             int which, bool inverse, const NttSealIn &s, u64 *part_out)
{
    const SealIoArgs sp{win, wout, wout8, logn / 2, sum_in, sum_out, s.part, part_out, s.hit_row, s.hit_coeff, s.hit_mask};
    return inverse ? launch_ntt_sealed_dir<true>(st, a, sp, logn, path, which, s) : launch_ntt_sealed_dir<false>(st, a, sp, logn, path, which, s);
}

} // namespace fhe
