// fourstep_checked.hip -- gfx950 kernels of the checked natural-order (four-step) transform: the two launches of launch_ntt_gs
// (ntt_kernels.hip) with the weighted checksums of abft_taps.hpp GsTap riding on the passes.  Launch 1 (the gathering inverse row
// pass) accumulates sum u x from the registers its first register step takes from the staged tile and sum m z from the lazy words
// it is about to store; launch 2 (the inverse column pass) sum m z from the hand-off words it has just loaded and sum v y from the
// canonical words it is about to store.  Each workgroup stores its canonical partial sums in the vector's row of a
// [vectors][tiles] array; launch_compare_sums / launch_compare_phases (aux_kernels.hip) add the rows up and write the flags.
// The words stored are those of the unchecked launches, bit for bit: the taps only read registers.
#include "ntt_launch.hpp"
#include "ntt_plan.hpp"
#include "abft_taps.hpp"

namespace fhe {

// test hook of the per-phase form: one bit of one word of the workgroup's LDS image between two register steps
template <class PASS>
FHE_D void gs_lds_fault(const GsCheckArgs &g, int pass, typename PASS::elem *lds)
{
    if (g.fault_pass == pass && g.fault_block == blockIdx.x) {
        if (threadIdx.x == 0) reinterpret_cast<u64 *>(lds)[g.fault_word % (u32)PASS::LDS_ELEMS] ^= (u64)1 << g.fault_bit;
        __syncthreads();
    }
}

// k_ntt_gs_first with the taps: one modulus (a.limbs == 1), unit = vector.  Phase 0 stages the tile (gather_in), the register
// steps follow; the hook sits between the first two of them (a flip before the first one would be a fault in the input).
template <class PASS, int LOGN, bool WA, bool WB>
__global__ __launch_bounds__(NTT_THREADS) void k_gs_first_checked(PassArgs a, GsCheckArgs g)
{
    typedef typename PASS::Arith A;
    typedef GsTap<A, 0, PASS::P, PASS::S0, WA, WB> Tap;
    static_assert(PASS::NPHASE >= 3, "a staging phase and at least two register steps");
    __shared__ __attribute__((aligned(16))) typename PASS::elem lds[PASS::LDS_ELEMS];
    __shared__ u64 red[2][NTT_THREADS / 64];
    const u32 unit = blockIdx.x / PASS::TILES, tile = blockIdx.x % PASS::TILES;
    const size_t off = (size_t)unit << LOGN;
    const LimbParams &p = a.lp[a.limb0];
    const typename A::Ctx ctx = A::make_ctx(p);
    const TwPtr tw = as_global(p.inv);
    const Tw inv_n = p.inv_n;
    const int tid = threadIdx.x;
    const u32 row0 = tile * PASS::TROWS;
    u64 *base = a.data + off;
    const u64 *from = a.src + off;
    Tap tap{as_global(g.u), as_global(g.m), as_global(g.v), (const u64 FHE_GLOBAL *)g.u8, (const u64 FHE_GLOBAL *)g.m8, row0, g.logp,
            typename A::elem(0), typename A::elem(0), 0, 0};
    PASS::template phase<0>(tid, base, lds, tw, row0, ctx, inv_n, &tap, from, 0u, nullptr, a.stream_hint != 0);
    __syncthreads();
    PASS::template phase<1>(tid, base, lds, tw, row0, ctx, inv_n, &tap);
    __syncthreads();
    gs_lds_fault<PASS>(g, 0, lds);
    PASS::template phase<2>(tid, base, lds, tw, row0, ctx, inv_n, &tap);
    if constexpr (PASS::NPHASE > 3) {
        __syncthreads();
        PASS::template phase<3>(tid, base, lds, tw, row0, ctx, inv_n, &tap);
    }
    if constexpr (WA) block_sum_mod(A::canonical(tap.acc_a, ctx), p.q, g.sum_a + (size_t)unit * PASS::TILES + tile, red[0]);
    if constexpr (WB) block_sum_mod(A::canonical(tap.acc_b, ctx), p.q, g.sum_b + (size_t)unit * PASS::TILES + tile, red[1]);
}

// the inverse column pass of launch 2 with the taps; a.src = the hand-off buffer (same layout as a.data)
template <class PASS, int LOGN, int P, bool WA, bool WB>
__global__ __launch_bounds__(NTT_THREADS) void k_gs_second_checked(PassArgs a, GsCheckArgs g)
{
    typedef typename PASS::Arith A;
    typedef GsTap<A, 1, P, LOGN - P, WA, WB> Tap;
    static_assert(PASS::NPHASE == 2 || PASS::NPHASE == 3, "two or three register steps");
    __shared__ __attribute__((aligned(16))) typename PASS::elem lds[PASS::LDS_ELEMS];
    __shared__ u64 red[2][NTT_THREADS / 64];
    u32 limb;
    u64 *base = col_tile<PASS, LOGN>(blockIdx.x, a, limb);
    const u32 unit = blockIdx.x / PASS::TILES, tile = blockIdx.x % PASS::TILES;
    const u32 pos0 = (u32)((base - a.data) & (((size_t)1 << LOGN) - 1));
    const LimbParams &p = a.lp[limb];
    const typename A::Ctx ctx = A::make_ctx(p);
    const TwPtr tw = as_global(p.inv);
    const Tw inv_n = p.inv_n;
    const int tid = threadIdx.x;
    const u64 *from = a.src + (base - a.data);
    Tap tap{as_global(g.u), as_global(g.m), as_global(g.v), (const u64 FHE_GLOBAL *)g.u8, (const u64 FHE_GLOBAL *)g.m8, pos0, g.logp,
            typename A::elem(0), typename A::elem(0), 0, 0};
    PASS::template phase<0>(tid, base, lds, tw, 0u, ctx, inv_n, &tap, from);
    __syncthreads();
    gs_lds_fault<PASS>(g, 1, lds);
    PASS::template phase<1>(tid, base, lds, tw, 0u, ctx, inv_n, &tap);
    if constexpr (PASS::NPHASE > 2) {
        __syncthreads();
        PASS::template phase<2>(tid, base, lds, tw, 0u, ctx, inv_n, &tap);
    }
    if constexpr (WA) block_sum_mod(A::canonical(tap.acc_a, ctx), p.q, g.sum_a + (size_t)unit * PASS::TILES + tile, red[0]);
    if constexpr (WB) block_sum_mod(A::canonical(tap.acc_b, ctx), p.q, g.sum_b + (size_t)unit * PASS::TILES + tile, red[1]);
}

template <class A, int LOGN>
static hipError_t launch_gs_checked_t(hipStream_t st, const PassArgs &a, u64 *tmp, const GsCheckArgs &c1, const GsCheckArgs &c2, bool phases, int which)
{
    typedef GsPasses<A, LOGN> GP;
    typedef typename GP::First First;
    const dim3 g1(a.units * First::TILES), th(NTT_THREADS);
    if constexpr (!GP::TWO) {
        if (which == 1) return hipSuccess;
        hipLaunchKernelGGL((k_gs_first_checked<First, LOGN, true, true>), g1, th, 0, st, a, c1);
        return hipGetLastError();
    } else {
        if (!tmp) return hipErrorInvalidValue;
        constexpr int P = First::P;
        typedef typename GP::Second Col;
        typedef typename GP::SecondNt ColNt;
        PassArgs first = a, second = a;
        first.data = tmp;
        second.src = tmp;
        const dim3 g2(a.units * Col::TILES);
        if (which != 1) {
            if (phases) hipLaunchKernelGGL((k_gs_first_checked<First, LOGN, true, true>), g1, th, 0, st, first, c1);
            else hipLaunchKernelGGL((k_gs_first_checked<First, LOGN, true, false>), g1, th, 0, st, first, c1);
        }
        if (which != 0) {
            if (a.stream_hint) {
                if (phases) hipLaunchKernelGGL((k_gs_second_checked<ColNt, LOGN, P, true, true>), g2, th, 0, st, second, c2);
                else hipLaunchKernelGGL((k_gs_second_checked<ColNt, LOGN, P, false, true>), g2, th, 0, st, second, c2);
            } else {
                if (phases) hipLaunchKernelGGL((k_gs_second_checked<Col, LOGN, P, true, true>), g2, th, 0, st, second, c2);
                else hipLaunchKernelGGL((k_gs_second_checked<Col, LOGN, P, false, true>), g2, th, 0, st, second, c2);
            }
        }
        return hipGetLastError();
    }
}

template <int LOGN> static void gs_checked_tiles_t(u32 *t1, u32 *t2)
{
    typedef GsPasses<ArithF64, LOGN> GP;
    *t1 = GP::First::TILES;
    if constexpr (GP::TWO) *t2 = GP::Second::TILES;
    else *t2 = 1;
}

void ntt_gs_checked_tiles(int logn, u32 *t1, u32 *t2)
{
    *t1 = *t2 = 1;
    switch (logn) {
#define FHE_CASE(L) case L: gs_checked_tiles_t<L>(t1, t2); break;
        FHE_CASE(5) FHE_CASE(6) FHE_CASE(7) FHE_CASE(8) FHE_CASE(9) FHE_CASE(10) FHE_CASE(11) FHE_CASE(12) FHE_CASE(13)
        FHE_CASE(14) FHE_CASE(15) FHE_CASE(16) FHE_CASE(17) FHE_CASE(18) FHE_CASE(19) FHE_CASE(20)
#undef FHE_CASE
    default: break;
    }
}

hipError_t launch_ntt_gs_checked(hipStream_t st, const PassArgs &a, u64 *tmp, const GsCheckArgs &c1, const GsCheckArgs &c2, int logn, int path,
                                 bool phases, int which)
{
    if (a.units == 0) return hipSuccess;
    if (!a.src || a.map || a.limbs != 1 || !ntt_gs_supported(logn) || (phases && logn < 13)) return hipErrorInvalidValue;
    switch (logn) {
#define FHE_CASE(L) \
    case L: return path == PATH_F64 ? launch_gs_checked_t<ArithF64, L>(st, a, tmp, c1, c2, phases, which) : launch_gs_checked_t<ArithU64, L>(st, a, tmp, c1, c2, phases, which);
        FHE_CASE(5) FHE_CASE(6) FHE_CASE(7) FHE_CASE(8) FHE_CASE(9) FHE_CASE(10) FHE_CASE(11) FHE_CASE(12) FHE_CASE(13)
        FHE_CASE(14) FHE_CASE(15) FHE_CASE(16) FHE_CASE(17) FHE_CASE(18) FHE_CASE(19) FHE_CASE(20)
#undef FHE_CASE
    default: return hipErrorInvalidValue;
    }
}

} // namespace fhe
