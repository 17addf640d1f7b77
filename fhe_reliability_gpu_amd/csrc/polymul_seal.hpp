// polymul_seal.hpp -- the single-launch negacyclic product with its factors' seals verified on the loads that transform them and
// its result sealed from the words it stores (host + device: k_polymul_mid_sealed of polymul_sealed.hip and the CPU emulation
// tests/emu/emu_polymul_seal.cpp compile the same steps with the same taps and the same pass templates).
//
// Below 2^13 the middle launch of the product is the whole product (ntt_kernels.hip k_polymul_mid; polymul_checked.hip
// k_polymul_mid_checked carries the detector's sums).  PolymulSealMid is k_polymul_mid_checked's body cut at its barriers into
// steps: the forward row steps of a, a's tile into registers, the forward row steps of b, the multiply with ProductSums and the
// point-2 test fault, the inverse row steps -- arithmetic, sums and the lazy hand-off through the LDS image unchanged.  What
// changes is the taps (ntt_seal_tap.hpp):
//   a, b   SealPassTap<A, false, HOOK, true, false>: besides sum w a / sum w b, every raw 64-bit word the first register step takes
//          is digested (weight = its index in the row plus one) and held against the window BEFORE it is converted;
//   c      the inverse-direction tap, with DIGEST when OUT: besides sum w c, every final word is digested on its way to memory.
// A lane therefore carries two input SealAccs with their range counts and, when OUT, one output SealAcc next to ra[PER][2].
// The kernel runs the steps with one barrier between two of them; the emulation runs each step for every thread in turn.
// Not covered: a fault between raw()'s read of a register and the conversion that consumes the same register.
#pragma once
#include "ntt_plan.hpp"
#include "ntt_seal_tap.hpp"

namespace fhe {

template <class A, int LOGN, int GEO, bool OUT, bool HOOK>
struct PolymulSealMid {
    typedef MidPasses<A, LOGN, GEO> MP;
    typedef typename MP::Fwd FR;
    typedef typename MP::Inv IR;
    static_assert(!MP::TWO, "two-launch sizes keep k_polymul_mid_checked: their column passes carry the taps");
    static_assert(FR::STAGED && IR::STAGED && FR::LDS_ELEMS == IR::LDS_ELEMS, "fused product needs the staged row pass");
    typedef typename FR::elem elem;
    typedef SealPassTap<A, false, HOOK, true, false> InTap;
    typedef SealPassTap<A, true, false, false, true, OUT> OutTap;
    static constexpr int PAIRS = FR::TROWS * FR::NPTS / 2;
    static constexpr int PER = (PAIRS + NTT_THREADS - 1) / NTT_THREADS;
    static constexpr int NFWD = FR::NSTEP, NINV = IR::NPHASE - 1;
    static constexpr int NSTEPS = 2 * NFWD + 2 + NINV;

    // what every lane of the workgroup shares: the tile's first words, its LDS image, the limb and the output-side weights
    struct Tile {
        u64 *a, *b, *c;
        elem *lds;
        const LimbParams *p;
        Tw inv_n;
        u32 row0;
        TwPtr wt;                       // w^ from the tile's first word on, twiddle encoding (ArithU64)
        const u64 FHE_GLOBAL *w8;       // the same as residues (ArithF64)
        int fk, fault_bit;              // point-2 test fault: local index of the product value to corrupt (-1: none)
    };
    struct Lane {
        InTap ta, tb;
        OutTap tc;
        ProductSums<A> ps;
        elem ra[PER][2];
    };

    // hit_a / hit_b: the hooked word's index relative to the tile's first word (NTT_SEAL_NO_HIT: none)
    static FHE_D Lane lane(TwPtr win, TwPtr wout, const u64 FHE_GLOBAL *wout8, u32 pos0, int logp, u64 q, u32 hit_a, u32 hit_b, u64 hit_mask)
    {
        return Lane{InTap{{win, wout, wout8, pos0, logp, elem(0), elem(0), 0, 0}, SealAcc{}, 0u, q, hit_a, hit_mask, SealAcc{}},
                    InTap{{win, wout, wout8, pos0, logp, elem(0), elem(0), 0, 0}, SealAcc{}, 0u, q, hit_b, hit_mask, SealAcc{}},
                    OutTap{{win, wout, wout8, pos0, logp, elem(0), elem(0), 0, 0}, SealAcc{}, 0u, q, NTT_SEAL_NO_HIT, 0, SealAcc{}},
                    ProductSums<A>{elem(0), elem(0), elem(0), 0},
                    {}};
    }

    // a's transformed tile (the arithmetic's lazy form) from the LDS image into the lane's registers
    static FHE_D void take(int tid, const elem *lds, elem (&ra)[PER][2])
    {
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
    }

    // b's tile multiplied in place in the LDS image, the detector's sums formed next to the product
    static FHE_D void multiply(int tid, const Tile &t, const typename A::Ctx &ctx, const elem (&ra)[PER][2], ProductSums<A> &ps)
    {
        const LimbParams &p = *t.p;
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const int i = tid + j * NTT_THREADS;
            if (PAIRS % NTT_THREADS == 0 || i < PAIRS) {
                const u32 row = (u32)i / (FR::NPTS / 2), g = ((u32)i % (FR::NPTS / 2)) * 2;
                const u32 e = row * FR::NPTS + g;          // the pair's position in the tile = in the weight table from the tile's first word
                elem *dst = t.lds + row * FR::ROW_LDS + row_pad(g);
                if constexpr (A::PATH == PATH_F64) {
                    ps.add(ra[j][0], dst[0], A::from_canonical(t.w8[e]), ctx);
                    ps.add(ra[j][1], dst[1], A::from_canonical(t.w8[e + 1]), ctx);
                    dst[0] = A::mulvar_lazy(ra[j][0], dst[0], ctx);
                    dst[1] = A::mulvar_lazy(ra[j][1], dst[1], ctx);
                } else {
                    ps.add(ra[j][0], dst[0], t.wt[e], ctx, p);
                    ps.add(ra[j][1], dst[1], t.wt[e + 1], ctx, p);
                    dst[0] = A::mulvar_lazy(ra[j][0], dst[0], p);
                    dst[1] = A::mulvar_lazy(ra[j][1], dst[1], p);
                }
                if (__builtin_expect(t.fk >= 0, 0) && (u32)i == (u32)t.fk >> 1) {
                    // a different residue in the same lazy range: flip the bit of the canonical value, reduce
                    elem &x = dst[t.fk & 1];
                    x = A::from_canonical((A::canonical(x, ctx) ^ ((u64)1 << t.fault_bit)) % p.q);
                }
            }
        }
    }

    // step S of NSTEPS for one thread; the steps are separated by a barrier
    template <int S> static FHE_D void step(int tid, const Tile &t, const typename A::Ctx &ctx, Lane &l)
    {
        if constexpr (S < NFWD) FR::template phase<S>(tid, t.a, t.lds, as_global(t.p->fwd), t.row0, ctx, t.inv_n, &l.ta);
        else if constexpr (S == NFWD) take(tid, t.lds, l.ra);
        else if constexpr (S <= 2 * NFWD) FR::template phase<S - NFWD - 1>(tid, t.b, t.lds, as_global(t.p->fwd), t.row0, ctx, t.inv_n, &l.tb);
        else if constexpr (S == 2 * NFWD + 1) multiply(tid, t, ctx, l.ra, l.ps);
        else IR::template phase<S - 2 * NFWD - 1>(tid, t.c, t.lds, as_global(t.p->inv), t.row0, ctx, t.inv_n, &l.tc);
    }
};

} // namespace fhe
