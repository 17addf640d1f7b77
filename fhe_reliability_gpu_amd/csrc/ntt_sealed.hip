// ntt_sealed.hip -- the checked inverse transform with its input's seal verified on the transform's own load (ntt_seal_tap.hpp):
// fhe_ntt_inverse_sealed and stage 0 of fhe_keyswitch_apply_sealed_in / fhe_rotate_sealed_in.  A translation unit of its own, so
// that every other kernel compiles exactly as before.
//
// k_ntt_pass_sealed is k_ntt_pass_abft's first launch of the checked inverse (ntt_kernels.hip: the inverse row pass of the
// two-launch sizes, the single pass below 2^13, where it also carries the output-side ABFT sum) with SealInTap in place of
// InvChecksumTap: every 64-bit word the first register step takes is digested -- weight = its index in the row plus one -- and
// held against the window before it is converted and enters the butterflies.  The pass loads from a.src when set (mirrored
// layout): an out-of-place transform with no copy between the seal's verification and the consuming load.  After the phases the
// workgroup stores its ABFT partial as k_ntt_pass_abft does and combines the lanes' SealAcc and range count through wave shuffles
// and 96 bytes of LDS into one integer partial {S0, S1, n_range} per (row, tile).
//
// k_ntt_seal_finish, one lane per row: merges the tiles' partials, holds the canonical (S0, S1) word for word against
// seal_src[row] (SEAL_SUM; a null seal pointer is not compared), raises SEAL_RANGE where a word was >= q_l, and stores the row's
// flag word.
//
// The second launch of the two-launch sizes (the inverse column pass with the output-side ABFT sum) is the checked inverse's own
// kernel, through launch_ntt_checked(which = 1).
//
// Integer arithmetic modulo 2^61 - 1 throughout the digest: no result depends on the grid or on the order of any combination.  No
// scratch memory, vector stores only, no atomics.  HOOK: the one-shot test fault of fhe_ctx_inject_fault_ntt_sealed, applied in
// the register (SealInTap::raw); memory stays clean.  Resources per instantiation: profiles/r20_ntt_sealed.md.
#include "ntt_launch.hpp"
#include "ntt_plan.hpp"
#include "ntt_seal_tap.hpp"

namespace fhe {

namespace {

struct SealPassArgs {
    const Tw *win, *wout;
    const u64 *wout8;
    int logp;
    u64 *sum_in, *sum_out;
    u64 *part;            // [rows][tiles][NTT_SEAL_PART]
    u32 hit_row, hit_coeff;
    u64 hit_mask;
};

} // namespace

// PASS: the inverse row pass (OUT = false) or the inverse single pass (OUT = true: it stores the final words too)
template <class PASS, int LOGN, bool HOOK, bool OUT>
__global__ __launch_bounds__(NTT_THREADS) void k_ntt_pass_sealed(PassArgs a, SealPassArgs s)
{
    typedef typename PASS::Arith A;
    typedef SealInTap<A, HOOK, OUT> Tap;
    __shared__ __attribute__((aligned(16))) typename PASS::elem lds[PASS::LDS_ELEMS];
    __shared__ u64 red[2][NTT_THREADS / 64];
    __shared__ u64 sred[NTT_THREADS / 64][NTT_SEAL_PART];
    u32 limb, row0 = 0;
    u64 *base = row_tile<PASS, LOGN>(blockIdx.x, a, limb, row0);
    // position of the tile inside its limb and index of the row in [poly][limb] order, as k_ntt_pass_abft
    const u32 unit = blockIdx.x / PASS::TILES, tile = blockIdx.x % PASS::TILES, polys = a.units / a.limbs;
    const u32 l = unit / polys, poly = unit % polys, slot = poly * a.poly_stride + l;
    const u32 pos0 = (u32)((base - a.data) & (((size_t)1 << LOGN) - 1));
    const LimbParams &p = a.lp[limb];
    const typename A::Ctx ctx = A::make_ctx(p);
    const TwPtr tw = as_global(p.inv);
    const Tw inv_n = p.inv_n;
    const int tid = threadIdx.x;
    const u32 hit_idx = HOOK && slot == s.hit_row && s.hit_coeff - pos0 < (u32)(PASS::TROWS * PASS::NPTS) ? s.hit_coeff - pos0 : NTT_SEAL_NO_HIT;
    Tap tap{{as_global(s.win) + ((size_t)limb << LOGN) + pos0, as_global(s.wout) + ((size_t)limb << LOGN) + pos0,
             (const u64 FHE_GLOBAL *)s.wout8 + ((size_t)limb << LOGN) + pos0, pos0, s.logp, typename A::elem(0), typename A::elem(0), 0, 0},
            SealAcc{}, 0u, p.q, hit_idx, s.hit_mask};
    const u64 *from = a.src ? a.src + (base - a.data) : nullptr;      // out of place: the consuming load reads the sealed rows themselves
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
    block_sum_mod(A::canonical(tap.acc_in, ctx), p.q, s.sum_in + (size_t)slot * PASS::TILES + tile, red[0]);
    if constexpr (OUT) block_sum_mod(A::canonical(tap.acc_out, ctx), p.q, s.sum_out + (size_t)slot * PASS::TILES + tile, red[1]);
    // the tile's digest: lanes -> wave -> workgroup, integers modulo 2^61 - 1 and a plain count
    SealAcc acc = tap.seal;
    u64 nr = tap.n_range;
    for (int o = 32; o; o >>= 1) {
        const u64 o0 = __shfl_xor(acc.s0, o), o1 = __shfl_xor(acc.s1, o);
        acc.merge(o0, o1);
        nr += __shfl_xor(nr, o);
    }
    if ((tid & 63) == 0) {
        sred[tid >> 6][0] = acc.s0;
        sred[tid >> 6][1] = acc.s1;
        sred[tid >> 6][2] = nr;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < NTT_THREADS / 64; w++) {
            acc.merge(sred[w][0], sred[w][1]);
            nr += sred[w][2];
        }
        u64 *dst = s.part + ((size_t)slot * PASS::TILES + tile) * NTT_SEAL_PART;
        dst[0] = acc.s0;
        dst[1] = acc.s1;
        dst[2] = nr;
    }
}

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

namespace {

template <class PASS, int LOGN, bool OUT>
hipError_t launch_first(hipStream_t st, const PassArgs &a, const SealPassArgs &sp, const NttSealIn &s)
{
    const dim3 grid(a.units * PASS::TILES), th(NTT_THREADS);
    if (s.hit_mask) hipLaunchKernelGGL((k_ntt_pass_sealed<PASS, LOGN, true, OUT>), grid, th, 0, st, a, sp);
    else hipLaunchKernelGGL((k_ntt_pass_sealed<PASS, LOGN, false, OUT>), grid, th, 0, st, a, sp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_ntt_seal_finish(st, a, (u32)PASS::TILES, s);
}

template <class A, int LOGN>
hipError_t launch_sealed_inv_t(hipStream_t st, const PassArgs &a, const Tw *win, const Tw *wout, const u64 *wout8, u64 *sum_in, u64 *sum_out, int path, int which,
                               const NttSealIn &s)
{
    constexpr int GEO = LOGN >= 13 ? 1 : 0;
    typedef Passes<A, LOGN, true, GEO> PS;
    const SealPassArgs sp{win, wout, wout8, LOGN / 2, sum_in, sum_out, s.part, s.hit_row, s.hit_coeff, s.hit_mask};
    if constexpr (!PS::G::TWO_PASS) {
        if (which == 1) return hipSuccess;
        return launch_first<typename PS::Single, LOGN, true>(st, a, sp, s);
    } else {
        if (which != 1) {
            hipError_t e = launch_first<typename PS::Row, LOGN, false>(st, a, sp, s);
            if (e != hipSuccess) return e;
        }
        if (which != 0) {
            PassArgs second = a;      // the column pass works in place on what the row pass left in a.data
            second.src = nullptr;
            return launch_ntt_checked(st, second, win, wout, wout8, sum_in, sum_out, LOGN, path, 1, true);
        }
        return hipSuccess;
    }
}

} // namespace

size_t ntt_seal_part_words(u32 rows, int logn)
{
    u32 tin = 1, tout = 1;
    ntt_checked_tiles(logn, &tin, &tout, true);
    return (size_t)rows * tin * NTT_SEAL_PART;
}

hipError_t launch_ntt_sealed_inv(hipStream_t st, const PassArgs &a, const Tw *win, const Tw *wout, const u64 *wout8, u64 *sum_in, u64 *sum_out, int logn, int path,
                                 int which, const NttSealIn &s)
{
    if (a.units == 0) return hipSuccess;
    if (a.map || a.scratch || a.tmp || a.src_bcast || a.src_stride || a.stream_hint || a.galois || a.galois_copy || !s.part || !s.flags) return hipErrorInvalidValue;
    switch (logn) {
#define FHE_CASE(L)                                                                                                                  \
    case L:                                                                                                                          \
        return path == PATH_F64 ? launch_sealed_inv_t<ArithF64, L>(st, a, win, wout, wout8, sum_in, sum_out, path, which, s)        \
                                : launch_sealed_inv_t<ArithU64, L>(st, a, win, wout, wout8, sum_in, sum_out, path, which, s);
        FHE_CASE(5) FHE_CASE(6) FHE_CASE(7) FHE_CASE(8) FHE_CASE(9) FHE_CASE(10) FHE_CASE(11) FHE_CASE(12) FHE_CASE(13)
        FHE_CASE(14) FHE_CASE(15) FHE_CASE(16) FHE_CASE(17) FHE_CASE(18) FHE_CASE(19) FHE_CASE(20)
#undef FHE_CASE
    default: return hipErrorInvalidValue;
    }
}

} // namespace fhe
