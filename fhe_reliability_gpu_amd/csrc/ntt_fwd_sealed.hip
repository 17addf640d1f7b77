// ntt_fwd_sealed.hip -- the checked forward transform with its input's seal verified on the transform's own load and its output's
// seal written from the words it stores (ntt_seal_tap.hpp, ntt_sealed_io.hpp): fhe_ntt_forward_sealed.  A translation unit of its
// own, so that every other kernel compiles exactly as before.
//
// Two-launch sizes (N >= 2^13): the forward column pass with the input digest, k_ntt_seal_finish (ntt_sealed.hip, unchanged) for
// the input rows' verdicts, the forward row pass with the output digest.  Below 2^13 the single pass carries both.  Without an
// output seal the second launch is the checked transform's own kernel.
//
// k_ntt_seal_out_finish, one lane per row, runs after launch_compare_sums: it merges the row's output partials and writes
// seal_dst[row] by the poison rule (ntt_seal_tap.hpp ntt_seal_out) -- the canonical pair where the row's input verdict and its
// ABFT flag are both zero, {~0, ~0} otherwise.  A ROW WITH ANY RAISED FLAG LEAVES THE CALL WITH A SEAL THAT CAN NEVER VERIFY.
//
// Resources per instantiation: profiles/r22_ntt_fwd_sealed.md.
#include "ntt_sealed_io.hpp"

namespace fhe {

__global__ __launch_bounds__(256) void k_ntt_seal_out_finish(const u64 *part_out, u32 tiles, u32 rows, const u32 *flags_in, const u32 *flags_abft, u64 *seal_dst)
{
    for (u32 r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += gridDim.x * blockDim.x) {
        const u64 *pr = part_out + (size_t)r * tiles * NTT_SEAL_OUT_PART;
        SealAcc acc;
        for (u32 t = 0; t < tiles; t++) acc.merge(pr[(size_t)t * NTT_SEAL_OUT_PART], pr[(size_t)t * NTT_SEAL_OUT_PART + 1]);
        u64 out[2];
        ntt_seal_out(acc, flags_in[r], flags_abft[r], out);
        seal_dst[2 * (size_t)r] = out[0];
        seal_dst[2 * (size_t)r + 1] = out[1];
    }
}

hipError_t launch_ntt_seal_out_finish(hipStream_t st, const u64 *part_out, u32 tiles, u32 rows, const u32 *flags_in, const u32 *flags_abft, u64 *seal_dst)
{
    if (!rows) return hipSuccess;
    const u32 grid = (rows + 255) / 256;
    hipLaunchKernelGGL(k_ntt_seal_out_finish, dim3(grid < 1024 ? grid : 1024), dim3(256), 0, st, part_out, tiles, rows, flags_in, flags_abft, seal_dst);
    return hipGetLastError();
}

namespace {

template <class A, int LOGN>
hipError_t launch_sealed_fwd_t(hipStream_t st, const PassArgs &a, const SealIoArgs &sp, int path, int which, const NttSealIn &s)
{
    constexpr int GEO = LOGN >= 13 ? 1 : 0;
    typedef Passes<A, LOGN, false, GEO> PS;
    if constexpr (!PS::G::TWO_PASS) {
        if (which == 1) return hipSuccess;
        hipError_t e = launch_sealed_io<typename PS::Single, LOGN, false, false, true, true>(st, a, sp);
        return e != hipSuccess ? e : launch_ntt_seal_finish(st, a, (u32)PS::Single::TILES, s);
    } else {
        if (which != 1) {
            hipError_t e = launch_sealed_io<typename PS::Col, LOGN, true, false, true, false>(st, a, sp);
            if (e == hipSuccess) e = launch_ntt_seal_finish(st, a, (u32)PS::Col::TILES, s);
            if (e != hipSuccess) return e;
        }
        if (which != 0) {
            PassArgs second = a;      // the row pass works in place on what the column pass left in a.data
            second.src = nullptr;
            if (!sp.part_out) return launch_ntt_checked(st, second, sp.win, sp.wout, sp.wout8, sp.sum_in, sp.sum_out, LOGN, path, 1, false);
            return launch_sealed_io<typename PS::Row, LOGN, false, false, false, true>(st, second, sp);
        }
        return hipSuccess;
    }
}

} // namespace

size_t ntt_seal_fwd_part_words(u32 rows, int logn)
{
    u32 tin = 1, tout = 1;
    ntt_checked_tiles(logn, &tin, &tout, false);
    return (size_t)rows * tin * NTT_SEAL_PART;
}

size_t ntt_seal_out_part_words(u32 rows, int logn, bool inverse)
{
    u32 tin = 1, tout = 1;
    ntt_checked_tiles(logn, &tin, &tout, inverse);
    return (size_t)rows * tout * NTT_SEAL_OUT_PART;
}

hipError_t launch_ntt_sealed_fwd(hipStream_t st, const PassArgs &a, const Tw *win, const Tw *wout, const u64 *wout8, u64 *sum_in, u64 *sum_out, int logn, int path,
                                 int which, const NttSealIn &s, u64 *part_out)
{
    if (a.units == 0) return hipSuccess;
    if (a.map || a.scratch || a.tmp || a.src_bcast || a.src_stride || a.stream_hint || a.galois || a.galois_copy || !s.part || !s.flags) return hipErrorInvalidValue;
    const SealIoArgs sp{win, wout, wout8, logn / 2, sum_in, sum_out, s.part, part_out, s.hit_row, s.hit_coeff, s.hit_mask};
    switch (logn) {
#define FHE_CASE(L) \
    case L: return path == PATH_F64 ? launch_sealed_fwd_t<ArithF64, L>(st, a, sp, path, which, s) : launch_sealed_fwd_t<ArithU64, L>(st, a, sp, path, which, s);
        FHE_CASE(5) FHE_CASE(6) FHE_CASE(7) FHE_CASE(8) FHE_CASE(9) FHE_CASE(10) FHE_CASE(11) FHE_CASE(12) FHE_CASE(13)
        FHE_CASE(14) FHE_CASE(15) FHE_CASE(16) FHE_CASE(17) FHE_CASE(18) FHE_CASE(19) FHE_CASE(20)
#undef FHE_CASE
    default: return hipErrorInvalidValue;
    }
}

} // namespace fhe
