// ntt_sealed_io.hpp -- the one pass kernel and the one launcher behind every sealed transform: fhe_ntt_inverse_sealed, stage 0 of
// fhe_keyswitch_apply_sealed_in / fhe_rotate_sealed_in, fhe_ntt_forward_sealed and fhe_ntt_inverse_sealed_out.  Device code:
// included by ntt_sealed.hip (inverse) and ntt_fwd_sealed.hip (forward) only, one direction each so that the two compile side by
// side, and so that every other kernel compiles exactly as before.
//
// k_ntt_pass_sealed_io is k_ntt_pass_abft (ntt_kernels.hip) with SealPassTap (ntt_seal_tap.hpp) in place of the ABFT tap:
//   IN      the launch that loads the transform's input -- every 64-bit word the first register step takes is digested (weight =
//           its index in the row plus one) and held against the window before it is converted; the pass loads from a.src when set
//           (mirrored layout): an out-of-place transform with no copy between the seal's verification and the consuming load;
//   OUT     the launch that stores the result forms the output-side ABFT sum;
//   DIGEST  it also digests every final word on its way to memory with weight = its index in the stored row plus one.  OUT without
//           DIGEST is the inverse single pass of a call that writes no output seal.
// After the phases the workgroup stores its ABFT partials as k_ntt_pass_abft does and combines the lanes' SealAccs and range count
// through wave shuffles and LDS into one integer partial per (row, tile): {S0, S1, n_range} of the input at s.part, {S0, S1} of
// the output at s.part_out -- distinct regions, the single pass writes both.  Integer arithmetic modulo 2^61 - 1 throughout the
// digest: no result depends on the grid or on the order of any combination.  No scratch memory, vector stores only, no atomics.
// HOOK: the one-shot test fault of fhe_ctx_inject_fault_ntt_sealed, applied in the register (SealTap::raw); memory stays clean.
//
// launch_sealed_t is the one launch sequence: the sealed first launch (the column pass of the forward transform, the row pass of the
// inverse, the single pass below 2^13) with k_ntt_seal_finish for the rows' verdicts, then the storing launch -- the checked
// transform's own kernel through launch_ntt_checked(which = 1) without an output seal, the digesting pass with one.
// Resources per instantiation: profiles/r23_ntt_sealed_fold.md.
#pragma once
#include "ntt_launch.hpp"
#include "ntt_plan.hpp"
#include "ntt_seal_tap.hpp"

namespace fhe {

struct SealIoArgs {
    const Tw *win, *wout;
    const u64 *wout8;
    int logp;
    u64 *sum_in, *sum_out;
    u64 *part;            // [rows][tiles][NTT_SEAL_PART], IN
    u64 *part_out;        // [rows][tiles][NTT_SEAL_OUT_PART], DIGEST (null: the digest is dropped)
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
template <class PASS, int LOGN, bool IS_COL, bool INV, bool IN, bool OUT, bool HOOK, bool DIGEST = OUT>
__global__ __launch_bounds__(NTT_THREADS, PASS::Arith::PATH == PATH_F64 ? 4 : 1) void k_ntt_pass_sealed_io(PassArgs a, SealIoArgs s)
{
    typedef typename PASS::Arith A;
    static_assert(IN || !HOOK, "the hook flips a word the launch loads");
    static_assert(OUT || !DIGEST, "the output digest rides on the storing launch");
    __shared__ __attribute__((aligned(16))) typename PASS::elem lds[PASS::LDS_ELEMS > 0 ? PASS::LDS_ELEMS : 1];
    __shared__ u64 red[2][NTT_THREADS / 64];
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
    SealPassTap<A, INV, HOOK, IN, OUT, DIGEST> tap{
        {as_global(s.win) + ((size_t)limb << LOGN) + pos0, as_global(s.wout) + ((size_t)limb << LOGN) + pos0,
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
        __shared__ u64 sred_in[NTT_THREADS / 64][NTT_SEAL_PART];
        u64 v[NTT_SEAL_PART] = {tap.seal.s0, tap.seal.s1, tap.n_range};
        block_seal_store<NTT_SEAL_PART, 1>(v, sred_in, s.part + at * NTT_SEAL_PART);
    }
    if constexpr (DIGEST) {
        __shared__ u64 sred_out[NTT_THREADS / 64][NTT_SEAL_OUT_PART];
        u64 v[NTT_SEAL_OUT_PART] = {tap.seal_out.s0, tap.seal_out.s1};
        block_seal_store<NTT_SEAL_OUT_PART, 0>(v, sred_out, s.part_out ? s.part_out + at * NTT_SEAL_OUT_PART : nullptr);
    }
}

template <class PASS, int LOGN, bool IS_COL, bool INV, bool IN, bool OUT, bool DIGEST = OUT>
hipError_t launch_sealed_io(hipStream_t st, const PassArgs &a, const SealIoArgs &s)
{
    const dim3 grid(a.units * PASS::TILES), th(NTT_THREADS);
    if constexpr (IN) {
        if (s.hit_mask) {
            hipLaunchKernelGGL((k_ntt_pass_sealed_io<PASS, LOGN, IS_COL, INV, IN, OUT, true, DIGEST>), grid, th, 0, st, a, s);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((k_ntt_pass_sealed_io<PASS, LOGN, IS_COL, INV, IN, OUT, false, DIGEST>), grid, th, 0, st, a, s);
    return hipGetLastError();
}

template <class A, int LOGN, bool INV>
hipError_t launch_sealed_t(hipStream_t st, const PassArgs &a, const SealIoArgs &sp, int path, int which, const NttSealIn &s)
{
    constexpr int GEO = LOGN >= 13 ? 1 : 0;
    typedef Passes<A, LOGN, INV, GEO> PS;
    if constexpr (!PS::G::TWO_PASS) {
        if (which == 1) return hipSuccess;
        // without an output seal the inverse single pass forms no output digest; the forward one forms it and drops it
        constexpr auto sealing = launch_sealed_io<typename PS::Single, LOGN, false, INV, true, true, true>;
        constexpr auto plain = launch_sealed_io<typename PS::Single, LOGN, false, INV, true, true, !INV>;
        hipError_t e = (sp.part_out ? sealing : plain)(st, a, sp);
        return e != hipSuccess ? e : launch_ntt_seal_finish(st, a, (u32)PS::Single::TILES, s);
    } else {
        typedef std::conditional_t<INV, typename PS::Row, typename PS::Col> First;
        typedef std::conditional_t<INV, typename PS::Col, typename PS::Row> Second;
        if (which != 1) {
            hipError_t e = launch_sealed_io<First, LOGN, !INV, INV, true, false>(st, a, sp);
            if (e == hipSuccess) e = launch_ntt_seal_finish(st, a, (u32)First::TILES, s);
            if (e != hipSuccess) return e;
        }
        if (which != 0) {
            PassArgs second = a;      // the second pass works in place on what the first left in a.data
            second.src = nullptr;
            if (!sp.part_out) return launch_ntt_checked(st, second, sp.win, sp.wout, sp.wout8, sp.sum_in, sp.sum_out, LOGN, path, 1, INV);
            return launch_sealed_io<Second, LOGN, INV, INV, false, true>(st, second, sp);
        }
        return hipSuccess;
    }
}

// launch_ntt_sealed (ntt_sealed.hip) for one direction: each direction's translation unit instantiates its own
template <bool INV>
hipError_t launch_ntt_sealed_dir(hipStream_t st, const PassArgs &a, const SealIoArgs &sp, int logn, int path, int which, const NttSealIn &s)
{
    if (a.units == 0) return hipSuccess;
    if (a.map || a.scratch || a.tmp || a.src_bcast || a.src_stride || a.stream_hint || a.galois || a.galois_copy || !s.part || !s.flags) return hipErrorInvalidValue;
    switch (logn) {
#define FHE_CASE(L) \
    case L: return path == PATH_F64 ? launch_sealed_t<ArithF64, L, INV>(st, a, sp, path, which, s) : launch_sealed_t<ArithU64, L, INV>(st, a, sp, path, which, s);
        FHE_CASE(5) FHE_CASE(6) FHE_CASE(7) FHE_CASE(8) FHE_CASE(9) FHE_CASE(10) FHE_CASE(11) FHE_CASE(12) FHE_CASE(13)
        FHE_CASE(14) FHE_CASE(15) FHE_CASE(16) FHE_CASE(17) FHE_CASE(18) FHE_CASE(19) FHE_CASE(20)
#undef FHE_CASE
    default: return hipErrorInvalidValue;
    }
}
extern template hipError_t launch_ntt_sealed_dir<true>(hipStream_t, const PassArgs &, const SealIoArgs &, int, int, int, const NttSealIn &);
extern template hipError_t launch_ntt_sealed_dir<false>(hipStream_t, const PassArgs &, const SealIoArgs &, int, int, int, const NttSealIn &);

} // namespace fhe
