// polymul_sealed.hip -- gfx950 kernels and the launch sequence of the sealed negacyclic product (fhe_polymul_sealed): the factors'
// seals verified on the loads that transform them, the product sealed from the words the last launch stores (polymul_seal.hpp,
// ntt_seal_tap.hpp).  A translation unit of its own, so that the unchecked and the checked product compile exactly as without it.
//
// N >= 2^13: launch_polymul_checked's launch list with the sealed passes of ntt_sealed_io.hpp at its two ends -- the forward column
// pass of each factor with the input digest (launch_ntt_sealed, first launch of the forward direction) and k_ntt_seal_finish for that
// factor's verdicts, k_polymul_mid_checked unchanged, and the inverse column pass digesting every word it stores (launch_ntt_sealed,
// second launch of the inverse direction) when an output seal is asked for, the checked one otherwise.  No kernel is instantiated
// here for these sizes.
//
// 2^5 <= N < 2^13: k_polymul_mid_sealed, the steps of PolymulSealMid with one barrier between two of them.  After the ABFT partials
// the workgroup combines its digests through block_seal_store: {S0, S1, n_range} of a at part_a, the same of b at part_b, {S0, S1} of
// c at part_c -- integers modulo 2^61 - 1 and plain counts, vector stores, no atomics; nothing depends on the grid or on the order of
// a combination.  HOOK: the one-shot test fault of fhe_ctx_inject_fault_polymul_sealed, applied in the register (SealTap::raw).
// Resources per instantiation: profiles/r24_polymul_sealed.md.
#include "ntt_sealed_io.hpp"
#include "polymul_seal.hpp"

namespace fhe {

struct PolymulSealArgs {
    PassArgs a;     // a.data = first factor (tile mapping as for a row pass)
    u64 *b;         // second factor, same layout
    u64 *c;         // product (may alias either factor)
    const Tw *win, *wout;
    const u64 *wout8;
    int logp;
    PolymulSums s;
    const u64 *fault_at;     // test hook (point 2), as k_polymul_mid_checked takes it; nullptr = off
    int fault_bit;
    u64 *part_a, *part_b;    // [rows][tiles][NTT_SEAL_PART]
    u64 *part_c;             // [rows][tiles][NTT_SEAL_OUT_PART], OUT (null: the digest is dropped)
    u32 hit_row, hit_coeff;  // HOOK: word hit_coeff of row hit_row of a (hit_ops & 1) and / or of b (hit_ops & 2)
    u64 hit_mask;
    u32 hit_ops;
};

template <class M, int S = 0>
__device__ __forceinline__ void polymul_seal_steps(int tid, const typename M::Tile &t, const typename M::FR::Arith::Ctx &ctx, typename M::Lane &l)
{
    if constexpr (S < M::NSTEPS) {
        if (S > 0) __syncthreads();
        M::template step<S>(tid, t, ctx, l);
        polymul_seal_steps<M, S + 1>(tid, t, ctx, l);
    }
}

template <class A, int LOGN, int GEO, bool OUT, bool HOOK>
__global__ __launch_bounds__(NTT_THREADS) void k_polymul_mid_sealed(PolymulSealArgs k)
{
    typedef PolymulSealMid<A, LOGN, GEO, OUT, HOOK> M;
    typedef typename M::FR FR;
    typedef typename M::elem elem;
    __shared__ __attribute__((aligned(16))) elem lds[FR::LDS_ELEMS];
    __shared__ u64 red[6][NTT_THREADS / 64];
    __shared__ u64 sred_in[2][NTT_THREADS / 64][NTT_SEAL_PART];
    u32 limb, row0;
    u64 *ta = row_tile<FR, LOGN>(blockIdx.x, k.a, limb, row0);
    const size_t off = (size_t)(ta - k.a.data);
    const LimbParams &p = k.a.lp[limb];
    const typename A::Ctx ctx = A::make_ctx(p);
    const int tid = threadIdx.x;
    const u32 unit = blockIdx.x / FR::TILES, tile = blockIdx.x % FR::TILES, polys = k.a.units / k.a.limbs;
    const u32 slot = (unit % polys) * k.a.poly_stride + unit / polys;
    const u32 pos0 = (u32)(off & (((size_t)1 << LOGN) - 1));
    const size_t woff = ((size_t)limb << LOGN) + pos0;
    // test hooks: local index of the product value to corrupt (-1: none), local index of the factor word to flip as it is loaded
    const int fk = k.fault_at && k.fault_at >= ta && k.fault_at < ta + FR::TROWS * FR::NPTS ? (int)(k.fault_at - ta) : -1;
    u32 hit_a = NTT_SEAL_NO_HIT, hit_b = NTT_SEAL_NO_HIT;
    if constexpr (HOOK) {
        if (slot == k.hit_row) {
            const u32 at = ntt_seal_tile_hit<FR, false>(k.hit_coeff, pos0);
            if (k.hit_ops & 1u) hit_a = at;
            if (k.hit_ops & 2u) hit_b = at;
        }
    }
    const typename M::Tile t{ta, k.b + off, k.c + off, lds, &p, p.inv_n, row0, as_global(k.wout) + woff, (const u64 FHE_GLOBAL *)k.wout8 + woff, fk, k.fault_bit};
    typename M::Lane l = M::lane(as_global(k.win) + woff, as_global(k.wout) + woff, (const u64 FHE_GLOBAL *)k.wout8 + woff, pos0, k.logp, p.q, hit_a, hit_b, k.hit_mask);
    polymul_seal_steps<M>(tid, t, ctx, l);
    const size_t at = (size_t)slot * FR::TILES + tile;
    block_sum_mod(A::canonical(l.ps.acc_a, ctx), p.q, k.s.aout + at, red[0]);
    block_sum_mod(A::canonical(l.ps.acc_b, ctx), p.q, k.s.bout + at, red[1]);
    block_sum_mod(A::canonical(l.ps.acc_ab, ctx), p.q, k.s.cin + at, red[2]);
    block_sum_mod(A::canonical(l.ta.acc_in, ctx), p.q, k.s.ain + at, red[3]);
    block_sum_mod(A::canonical(l.tb.acc_in, ctx), p.q, k.s.bin + at, red[4]);
    block_sum_mod(A::canonical(l.tc.acc_out, ctx), p.q, k.s.cout + at, red[5]);
    // the tile's digests: lanes -> wave -> workgroup, integers modulo 2^61 - 1 and a plain count
    u64 va[NTT_SEAL_PART] = {l.ta.seal.s0, l.ta.seal.s1, l.ta.n_range};
    block_seal_store<NTT_SEAL_PART, 1>(va, sred_in[0], k.part_a + at * NTT_SEAL_PART);
    u64 vb[NTT_SEAL_PART] = {l.tb.seal.s0, l.tb.seal.s1, l.tb.n_range};
    block_seal_store<NTT_SEAL_PART, 1>(vb, sred_in[1], k.part_b + at * NTT_SEAL_PART);
    if constexpr (OUT) {
        __shared__ u64 sred_out[NTT_THREADS / 64][NTT_SEAL_OUT_PART];
        u64 vc[NTT_SEAL_OUT_PART] = {l.tc.seal_out.s0, l.tc.seal_out.s1};
        block_seal_store<NTT_SEAL_OUT_PART, 0>(vc, sred_out, k.part_c ? k.part_c + at * NTT_SEAL_OUT_PART : nullptr);
    }
}

template <class A, int LOGN>
static hipError_t launch_mid_sealed(hipStream_t st, const PolymulSealArgs &k)
{
    typedef typename MidPasses<A, LOGN, 0>::Fwd FR;
    const dim3 grid(k.a.units * FR::TILES), th(NTT_THREADS);
    if (k.hit_mask) {
        if (k.part_c) hipLaunchKernelGGL((k_polymul_mid_sealed<A, LOGN, 0, true, true>), grid, th, 0, st, k);
        else hipLaunchKernelGGL((k_polymul_mid_sealed<A, LOGN, 0, false, true>), grid, th, 0, st, k);
    } else if (k.part_c) hipLaunchKernelGGL((k_polymul_mid_sealed<A, LOGN, 0, true, false>), grid, th, 0, st, k);
    else hipLaunchKernelGGL((k_polymul_mid_sealed<A, LOGN, 0, false, false>), grid, th, 0, st, k);
    return hipGetLastError();
}

hipError_t launch_polymul_sealed(hipStream_t st, const PassArgs &a, u64 *b, u64 *c, int logn, int path, const PolymulChecks &k, const PolymulSealIo &io)
{
    if (a.units == 0) return hipSuccess;
    if (!polymul_fused_supported(logn) || a.map || a.scratch || a.tmp || a.src || a.src_bcast || a.src_stride || a.stream_hint || a.galois || a.galois_copy)
        return hipErrorInvalidValue;
    const bool square = b == a.data;
    if (!io.a.part || !io.a.flags || (!square && (!io.b.part || !io.b.flags))) return hipErrorInvalidValue;
    hipError_t e;
    if (logn >= 13) {
        PassArgs pb = a, pc = a;
        pb.data = b;
        pc.data = c;
        // the forward column pass of each factor with its input digest, then that factor's verdicts
        if ((e = launch_ntt_sealed(st, a, k.win, k.wout, k.wout8, k.s.ain, nullptr, logn, path, 0, false, io.a, nullptr)) != hipSuccess) return e;
        if (!square && (e = launch_ntt_sealed(st, pb, k.win, k.wout, k.wout8, k.s.bin, nullptr, logn, path, 0, false, io.b, nullptr)) != hipSuccess) return e;
        if ((k.fault_point == 0 || k.fault_point == 1) && (e = launch_flip_bit(st, k.fault_at, 0, k.fault_bit)) != hipSuccess) return e;
        if ((e = launch_polymul_mid_checked(st, a, b, c, logn, path, k)) != hipSuccess) return e;
        if (k.fault_point == 3 && (e = launch_flip_bit(st, k.fault_at, 0, k.fault_bit)) != hipSuccess) return e;
        // the inverse column pass: the digesting storing pass with an output seal, the checked transform's own kernel without
        NttSealIn none{nullptr, io.a.flags, io.a.part};      // (the second launch reads neither; launch_ntt_sealed asks for both)
        return launch_ntt_sealed(st, pc, k.win, k.wout, k.wout8, nullptr, k.s.cout, logn, path, 1, true, none, io.part_c);
    }
    const NttSealIn &h = io.a.hit_mask ? io.a : io.b;
    const u32 ops = io.a.hit_mask ? (square ? 3u : 1u) : io.b.hit_mask ? 2u : 0u;
    const PolymulSealArgs pk{a, b, c, k.win, k.wout, k.wout8, logn / 2, k.s, k.fault_point == 2 ? k.fault_at : nullptr, k.fault_bit,
                             io.a.part, square ? io.a.part : io.b.part, io.part_c, h.hit_row, h.hit_coeff, ops ? h.hit_mask : 0, ops};
    switch (logn) {
#define FHE_CASE(L)                                                                                                \
    case L:                                                                                                        \
        e = path == PATH_F64 ? launch_mid_sealed<ArithF64, L>(st, pk) : launch_mid_sealed<ArithU64, L>(st, pk);    \
        break;
        FHE_CASE(5) FHE_CASE(6) FHE_CASE(7) FHE_CASE(8) FHE_CASE(9) FHE_CASE(10) FHE_CASE(11) FHE_CASE(12)
#undef FHE_CASE
    default:
        return hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
    if ((e = launch_ntt_seal_finish(st, a, k.s.t_mid, io.a)) != hipSuccess) return e;
    return square ? hipSuccess : launch_ntt_seal_finish(st, a, k.s.t_mid, io.b);
}

} // namespace fhe
