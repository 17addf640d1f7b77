// polymul_checked.hip -- gfx950 kernels of the checked negacyclic product (fhe_polymul_checked): the middle launch of
// ntt_kernels.hip k_polymul_mid with the detector's sums, and the launch sequence around it.  A translation unit of its
// own, so that the unchecked product's kernels compile exactly as without it.
#include "ntt_launch.hpp"
#include "ntt_plan.hpp"
#include "abft_taps.hpp"

#include <type_traits>

namespace fhe {

// ntt_kernels.hip fwd_steps / inv_steps with a tap on the passes (NoTap at two-launch sizes, whose column passes carry the taps)
template <class FR, int E = 0, class TAP>
FHE_D void fwd_steps_tap(int tid, u64 *base, typename FR::elem *lds, TwPtr tw, u32 row0, const typename FR::Arith::Ctx &ctx, const Tw &inv_n, TAP *tap)
{
    if constexpr (E < FR::NSTEP) {
        if (E > 0) __syncthreads();
        FR::template phase<E, TAP>(tid, base, lds, tw, row0, ctx, inv_n, tap);
        fwd_steps_tap<FR, E + 1>(tid, base, lds, tw, row0, ctx, inv_n, tap);
    }
}
template <class IR, int E = 1, class TAP>
FHE_D void inv_steps_tap(int tid, u64 *base, typename IR::elem *lds, TwPtr tw, u32 row0, const typename IR::Arith::Ctx &ctx, const Tw &inv_n, TAP *tap)
{
    if constexpr (E < IR::NPHASE) {
        __syncthreads();
        IR::template phase<E, TAP>(tid, base, lds, tw, row0, ctx, inv_n, tap);
        inv_steps_tap<IR, E + 1>(tid, base, lds, tw, row0, ctx, inv_n, tap);
    }
}

// ---------------------------------------------------------------------------
// Checked product (ABFT around c = a * b, the protected chain of rfhe_framewk/src/four_step_ntt_protected.py:219-282:
// transform -> element-wise product -> transform, each with its own check).  The middle launch of k_polymul_mid with the
// sums of abft_taps.hpp ProductSums formed where the product is: per point, w^ a^ and w^ b^ close the forward checks of
// the factors and (w^ a^) b^ opens the product's check, closed by sum w c over the words the inverse column pass stores.
// One-launch sizes: the middle launch is the whole product, so it also carries the input taps (sum w a, sum w b on the
// loads of the forward row steps) and the output tap (sum w c on the stores of the inverse row steps).
// ---------------------------------------------------------------------------
struct PolymulChkArgs {
    PassArgs a;     // a.data = first factor (tile mapping as for a row pass)
    const u64 *b;   // second factor, same layout
    u64 *c;         // product (may alias either factor)
    const Tw *win, *wout;
    const u64 *wout8;
    int logp;
    PolymulSums s;
    const u64 *fault_at;     // test hook (point 2): the product value at this word's tile position (a's buffer) is flipped; nullptr = off
    int fault_bit;
};

template <class A, int LOGN, int GEO>
__global__ __launch_bounds__(NTT_THREADS) void k_polymul_mid_checked(PolymulChkArgs k)
{
    typedef MidPasses<A, LOGN, GEO> MP;
    typedef typename MP::Fwd FR;
    typedef typename MP::Inv IR;
    static_assert(FR::STAGED && IR::STAGED && FR::LDS_ELEMS == IR::LDS_ELEMS, "fused product needs the staged row pass");
    typedef typename FR::elem elem;
    typedef ChecksumTap<A, true, false> InTap;          // one-launch sizes: sum w a / sum w b on the loads
    typedef InvChecksumTap<A, false, true> OutTap;      // one-launch sizes: sum w c on the stores
    constexpr int PAIRS = FR::TROWS * FR::NPTS / 2;
    constexpr int PER = (PAIRS + NTT_THREADS - 1) / NTT_THREADS;
    const PolymulChkArgs &pa = k;
    __shared__ __attribute__((aligned(16))) elem lds[FR::LDS_ELEMS];
    __shared__ u64 red[6][NTT_THREADS / 64];
    u32 limb, row0;
    u64 *ta = row_tile<FR, LOGN>(blockIdx.x, pa.a, limb, row0);
    const size_t off = (size_t)(ta - pa.a.data);
    const LimbParams &p = pa.a.lp[limb];
    const typename A::Ctx ctx = A::make_ctx(p);
    const Tw inv_n = p.inv_n;
    const int tid = threadIdx.x;
    const u32 unit = blockIdx.x / FR::TILES, tile = blockIdx.x % FR::TILES, polys = pa.a.units / pa.a.limbs;
    const size_t slot = (size_t)(unit % polys) * pa.a.poly_stride + unit / polys;
    const u32 pos0 = (u32)(off & (((size_t)1 << LOGN) - 1));
    const size_t woff = ((size_t)limb << LOGN) + pos0;
    InTap tin_a{as_global(k.win) + woff, as_global(k.wout) + woff, (const u64 FHE_GLOBAL *)k.wout8 + woff, pos0, k.logp, elem(0), elem(0), 0, 0};
    InTap tin_b = tin_a;
    OutTap tout_c{as_global(k.win) + woff, as_global(k.wout) + woff, (const u64 FHE_GLOBAL *)k.wout8 + woff, pos0, k.logp, elem(0), elem(0), 0, 0};
    // test hook: local index of the product value to corrupt in this tile (-1: none)
    const int fk = k.fault_at && k.fault_at >= ta && k.fault_at < ta + FR::TROWS * FR::NPTS ? (int)(k.fault_at - ta) : -1;

    if constexpr (MP::TWO) fwd_steps_tap<FR>(tid, ta, lds, as_global(p.fwd), row0, ctx, inv_n, (NoTap *)nullptr);   // (the column pass carried the input tap)
    else fwd_steps_tap<FR>(tid, ta, lds, as_global(p.fwd), row0, ctx, inv_n, &tin_a);
    __syncthreads();
    elem ra[PER][2];
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const int i = tid + j * NTT_THREADS;
        if (PAIRS % NTT_THREADS == 0 || i < PAIRS) {
            const u32 row = (u32)i / (FR::NPTS / 2), g = ((u32)i % (FR::NPTS / 2)) * 2;
            const elem *src = lds + row * FR::ROW_LDS + row_pad(g);
            ra[j][0] = src[0];
            ra[j][1] = src[1];
        }
    }
    __syncthreads();
    if constexpr (MP::TWO) fwd_steps_tap<FR>(tid, const_cast<u64 *>(pa.b) + off, lds, as_global(p.fwd), row0, ctx, inv_n, (NoTap *)nullptr);   // (the column pass carried the input tap)
    else fwd_steps_tap<FR>(tid, const_cast<u64 *>(pa.b) + off, lds, as_global(p.fwd), row0, ctx, inv_n, &tin_b);
    __syncthreads();
    ProductSums<A> ps{elem(0), elem(0), elem(0), 0};
    const u64 FHE_GLOBAL *w8 = (const u64 FHE_GLOBAL *)k.wout8 + woff;
    const TwPtr wt = as_global(k.wout) + woff;
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const int i = tid + j * NTT_THREADS;
        if (PAIRS % NTT_THREADS == 0 || i < PAIRS) {
            const u32 row = (u32)i / (FR::NPTS / 2), g = ((u32)i % (FR::NPTS / 2)) * 2;
            const u32 e = row * FR::NPTS + g;          // the pair's position in the tile = in the weight table from woff
            elem *dst = lds + row * FR::ROW_LDS + row_pad(g);
            if constexpr (A::PATH == PATH_F64) {
                ps.add(ra[j][0], dst[0], A::from_canonical(w8[e]), ctx);
                ps.add(ra[j][1], dst[1], A::from_canonical(w8[e + 1]), ctx);
                dst[0] = A::mulvar_lazy(ra[j][0], dst[0], ctx);
                dst[1] = A::mulvar_lazy(ra[j][1], dst[1], ctx);
            } else {
                ps.add(ra[j][0], dst[0], wt[e], ctx, p);
                ps.add(ra[j][1], dst[1], wt[e + 1], ctx, p);
                dst[0] = A::mulvar_lazy(ra[j][0], dst[0], p);
                dst[1] = A::mulvar_lazy(ra[j][1], dst[1], p);
            }
            if (__builtin_expect(fk >= 0, 0) && (u32)i == (u32)fk >> 1) {
                // a different residue in the same lazy range: flip the bit of the canonical value, reduce
                elem &x = dst[fk & 1];
                x = A::from_canonical((A::canonical(x, ctx) ^ ((u64)1 << k.fault_bit)) % p.q);
            }
        }
    }
    if constexpr (MP::TWO) inv_steps_tap<IR>(tid, pa.c + off, lds, as_global(p.inv), row0, ctx, inv_n, (NoTap *)nullptr);   // (lazy hand-off)
    else inv_steps_tap<IR>(tid, pa.c + off, lds, as_global(p.inv), row0, ctx, inv_n, &tout_c);
    const size_t at = slot * FR::TILES + tile;
    block_sum_mod(A::canonical(ps.acc_a, ctx), p.q, k.s.aout + at, red[0]);
    block_sum_mod(A::canonical(ps.acc_b, ctx), p.q, k.s.bout + at, red[1]);
    block_sum_mod(A::canonical(ps.acc_ab, ctx), p.q, k.s.cin + at, red[2]);
    if constexpr (!MP::TWO) {
        block_sum_mod(A::canonical(tin_a.acc_in, ctx), p.q, k.s.ain + at, red[3]);
        block_sum_mod(A::canonical(tin_b.acc_in, ctx), p.q, k.s.bin + at, red[4]);
        block_sum_mod(A::canonical(tout_c.acc_out, ctx), p.q, k.s.cout + at, red[5]);
    }
}

template <class A, int LOGN>
static hipError_t launch_mid_checked(hipStream_t st, const PolymulChkArgs &k)
{
    constexpr int GEO = LOGN >= 13 ? 1 : 0;
    typedef typename MidPasses<A, LOGN, GEO>::Fwd FR;
    hipLaunchKernelGGL((k_polymul_mid_checked<A, LOGN, GEO>), dim3(k.a.units * FR::TILES), dim3(NTT_THREADS), 0, st, k);
    return hipGetLastError();
}

template <int LOGN> static void polymul_tiles_t(u32 *t_in, u32 *t_mid, u32 *t_out)
{
    constexpr int GEO = LOGN >= 13 ? 1 : 0;
    typedef MidPasses<ArithF64, LOGN, GEO> MP;
    *t_in = *t_mid = *t_out = MP::Fwd::TILES;
    if constexpr (MP::TWO) {
        *t_in = MP::F::Col::TILES;
        *t_out = MP::I::Col::TILES;
    }
}
// partial sums per unit of the checked product (row lengths of PolymulSums' arrays)
void polymul_checked_tiles(int logn, u32 *t_in, u32 *t_mid, u32 *t_out)
{
    *t_in = *t_mid = *t_out = 1;
    switch (logn) {
#define FHE_CASE(L) case L: polymul_tiles_t<L>(t_in, t_mid, t_out); break;
        FHE_CASE(5) FHE_CASE(6) FHE_CASE(7) FHE_CASE(8) FHE_CASE(9) FHE_CASE(10) FHE_CASE(11) FHE_CASE(12) FHE_CASE(13)
        FHE_CASE(14) FHE_CASE(15) FHE_CASE(16) FHE_CASE(17) FHE_CASE(18) FHE_CASE(19) FHE_CASE(20)
#undef FHE_CASE
    default: break;
    }
}

// the middle launch alone (fault point 2 honoured): what launch_polymul_checked runs between the column passes, and what the sealed
// product (polymul_sealed.hip) runs between its sealed ones at two-launch sizes
hipError_t launch_polymul_mid_checked(hipStream_t st, const PassArgs &a, u64 *b, u64 *c, int logn, int path, const PolymulChecks &k)
{
    const PolymulChkArgs pk{a, b, c, k.win, k.wout, k.wout8, logn / 2, k.s, k.fault_point == 2 ? k.fault_at : nullptr, k.fault_bit};
    switch (logn) {
#define FHE_CASE(L) \
    case L: return path == PATH_F64 ? launch_mid_checked<ArithF64, L>(st, pk) : launch_mid_checked<ArithU64, L>(st, pk);
        FHE_CASE(5) FHE_CASE(6) FHE_CASE(7) FHE_CASE(8) FHE_CASE(9) FHE_CASE(10) FHE_CASE(11) FHE_CASE(12) FHE_CASE(13)
        FHE_CASE(14) FHE_CASE(15) FHE_CASE(16) FHE_CASE(17) FHE_CASE(18) FHE_CASE(19) FHE_CASE(20)
#undef FHE_CASE
    default:
        return hipErrorInvalidValue;
    }
}

// launch_polymul with the detector: forward column passes with the input taps (two-launch sizes), the checked middle launch,
// inverse column pass with the output tap.  k.s's pointers are this launch's rows (the caller offsets them like the data).
hipError_t launch_polymul_checked(hipStream_t st, const PassArgs &a, u64 *b, u64 *c, int logn, int path, const PolymulChecks &k)
{
    if (a.units == 0) return hipSuccess;
    if (!polymul_fused_supported(logn) || a.map) return hipErrorInvalidValue;
    hipError_t e;
    PassArgs pb = a, pc = a;
    pb.data = b;
    pc.data = c;
    if (logn >= 13) {
        if ((e = launch_ntt_checked(st, a, k.win, k.wout, k.wout8, k.s.ain, nullptr, logn, path, 0)) != hipSuccess) return e;
        if (b != a.data && (e = launch_ntt_checked(st, pb, k.win, k.wout, k.wout8, k.s.bin, nullptr, logn, path, 0)) != hipSuccess) return e;
        if ((k.fault_point == 0 || k.fault_point == 1) && (e = launch_flip_bit(st, k.fault_at, 0, k.fault_bit)) != hipSuccess) return e;
    }
    if ((e = launch_polymul_mid_checked(st, a, b, c, logn, path, k)) != hipSuccess) return e;
    if (logn >= 13) {
        if (k.fault_point == 3 && (e = launch_flip_bit(st, k.fault_at, 0, k.fault_bit)) != hipSuccess) return e;
        return launch_ntt_checked(st, pc, k.win, k.wout, k.wout8, nullptr, k.s.cout, logn, path, 1, true);
    }
    return hipSuccess;
}

} // namespace fhe
