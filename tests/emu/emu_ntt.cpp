// emu_ntt.cpp -- CPU emulation of the HIP NTT passes (TEST INFRASTRUCTURE ONLY).
//
// Compiles fhe_reliability_gpu_amd/csrc/ntt_core.hpp / ntt_plan.hpp with g++ and
// runs every workgroup step as a loop over thread ids, so the tile indexing, the
// twiddle indexing, the LDS exchange pattern and the FP64 lazy-range schedule can be
// checked against the oracle without a GPU.  It is NOT a product path: the library
// never links this file.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I<csrc> emu_ntt.cpp -o libemu_ntt.so
#include "ntt_fused.hpp"

#include <array>
#include <cmath>
#include <utility>
#include <vector>

using namespace fhe;

namespace {

// Largest |value| (units of q) any FP64 register held where the arithmetic reads or produces it, and the largest pair sum
// |X| + |Y| an inverse butterfly was given: the lazy schedule keeps both at or below 8 (q < 2^50: exact integers below 2^53).
double g_max_ratio = 0.0, g_max_pair = 0.0;

// ArithF64 with every operand watched.  It delegates to ArithF64 unchanged, so the words are the kernels' words; what it adds is
// the view of the registers BEFORE a butterfly, a product or a fold, which no LDS image after a pass can give.
struct TrackF64 : ArithF64 {
    static void see(double x, const Ctx &c)
    {
        const double r = std::fabs(x) / c.n;
        if (!(r <= g_max_ratio)) g_max_ratio = r;          // (a NaN sticks)
    }
    static void see_pair(double x, double y, const Ctx &c)
    {
        const double r = (std::fabs(x) + std::fabs(y)) / c.n;
        if (!(r <= g_max_pair)) g_max_pair = r;
    }
    static void reduce(elem &x, const Ctx &c)
    {
        see(x, c);
        ArithF64::reduce(x, c);
    }
    static u64 canonical(elem x, const Ctx &c)
    {
        see(x, c);
        return ArithF64::canonical(x, c);
    }
    static elem mulmod(elem a, const Tw &t, const Ctx &c)
    {
        see(a, c);
        return ArithF64::mulmod(a, t, c);
    }
    static void bfly_fwd(elem &X, elem &Y, const Tw &t, const Ctx &c)
    {
        see(X, c), see(Y, c);
        ArithF64::bfly_fwd(X, Y, t, c);
        see(X, c), see(Y, c);
    }
    static void bfly_inv(elem &X, elem &Y, const Tw &t, const Ctx &c)
    {
        see(X, c), see(Y, c), see_pair(X, Y, c);
        ArithF64::bfly_inv(X, Y, t, c);
        see(X, c), see(Y, c);
    }
    static void bfly_inv_scaled(elem &X, elem &Y, const Tw &n, const Tw &wn, const Ctx &c)
    {
        see(X, c), see(Y, c), see_pair(X, Y, c);
        ArithF64::bfly_inv_scaled(X, Y, n, wn, c);
        see(X, c), see(Y, c);
    }
};

// What the integer path met (tests/test_emu_harvey_cases.py): equalities at its comparisons, Shoup products in the upper half, and
// operands outside the documented ranges.  Indices of emu_u64_events().
enum { EV_FOLD_EQ, EV_SUM_EQ, EV_FINAL_Q, EV_FINAL_2Q, EV_FINAL_3Q, EV_SHOUP_HI, EV_BARRETT_Q, EV_RANGE, EV_COUNT };
u64 g_ev[EV_COUNT];

// ArithU64 with every operand watched.  It delegates to ArithU64 unchanged, so the words are the kernels' words; the Shoup product a
// butterfly makes inside is made once more here (it is a pure function) only to be looked at.  The documented ranges -- operands
// below 4q forward, below 2q inverse, so that canonical() has at most 3q to remove -- are checked on every butterfly and counted
// in EV_RANGE instead of aborting, so that a test can say which input broke them.
struct TrackU64 : ArithU64 {
    static void shoup(elem a, const Tw &t, const Ctx &c)
    {
        const u64 r = ArithU64::mulmod(a, t, c);
        if (r >= c.two_q) g_ev[EV_RANGE]++;
        else if (r >= c.q) g_ev[EV_SHOUP_HI]++;
    }
    static u64 canonical(elem x, const Ctx &c)
    {
        if (x == c.q) g_ev[EV_FINAL_Q]++;
        if (x == c.two_q) g_ev[EV_FINAL_2Q]++;
        if (x == c.two_q + c.q) g_ev[EV_FINAL_3Q]++;
        if (x >= 2 * c.two_q) g_ev[EV_RANGE]++;
        return ArithU64::canonical(x, c);
    }
    static elem mulmod(elem a, const Tw &t, const Ctx &c)
    {
        shoup(a, t, c);
        return ArithU64::mulmod(a, t, c);
    }
    static void bfly_fwd(elem &X, elem &Y, const Tw &t, const Ctx &c)
    {
        if (X >= 2 * c.two_q || Y >= 2 * c.two_q) g_ev[EV_RANGE]++;
        if (X == c.two_q) g_ev[EV_FOLD_EQ]++;
        shoup(Y, t, c);
        ArithU64::bfly_fwd(X, Y, t, c);
        if (X >= 2 * c.two_q || Y >= 2 * c.two_q) g_ev[EV_RANGE]++;
    }
    static void inv_head(elem X, elem Y, const Ctx &c)
    {
        if (X >= c.two_q || Y >= c.two_q) g_ev[EV_RANGE]++;
        if (X + Y == c.two_q) g_ev[EV_SUM_EQ]++;
    }
    static void bfly_inv(elem &X, elem &Y, const Tw &t, const Ctx &c)
    {
        inv_head(X, Y, c);
        shoup(X - Y + c.two_q, t, c);
        ArithU64::bfly_inv(X, Y, t, c);
        if (X >= c.two_q || Y >= c.two_q) g_ev[EV_RANGE]++;
    }
    static void bfly_inv_scaled(elem &X, elem &Y, const Tw &n, const Tw &wn, const Ctx &c)
    {
        inv_head(X, Y, c);
        shoup(X + Y, n, c), shoup(X - Y + c.two_q, wn, c);
        ArithU64::bfly_inv_scaled(X, Y, n, wn, c);
        if (X >= c.two_q || Y >= c.two_q) g_ev[EV_RANGE]++;
    }
    // the quotient estimate of barrett128 once more: floor(x * floor(2^128 / q) / 2^128) for x = (hi:lo)
    static elem mulvar_lazy(elem a, elem b, const LimbParams &p)
    {
        if (a >= 2 * p.two_q || b >= 2 * p.two_q) g_ev[EV_RANGE]++;
        const u64 lo = a * b, hi = mulhi64(a, b), r0 = p.barrett_lo, r1 = p.barrett_hi;
        const unsigned __int128 mid = (unsigned __int128)lo * r1 + mulhi64(lo, r0);
        const unsigned __int128 mid2 = (unsigned __int128)hi * r0 + (u64)mid;
        const u64 qhat = hi * r1 + (u64)(mid >> 64) + (u64)(mid2 >> 64);
        if (lo - qhat * p.q == p.q) g_ev[EV_BARRETT_Q]++;
        return ArithU64::mulvar_lazy(a, b, p);
    }
};

template <class PASS, int LOGN, bool INV, bool IS_COL>
void emu_pass(const PassArgs &a)
{
    typedef typename PASS::Arith A;
    const u32 blocks = a.units * PASS::TILES;
    std::vector<typename PASS::elem> lds(PASS::LDS_ELEMS > 0 ? PASS::LDS_ELEMS : 1);
    for (u32 b = 0; b < blocks; b++) {
        u32 limb, row0 = 0;
        u64 *base;
        if constexpr (IS_COL) base = col_tile<PASS, LOGN>(b, a, limb);
        else base = row_tile<PASS, LOGN>(b, a, limb, row0);
        const LimbParams &p = a.lp[limb];
        auto ctx = A::make_ctx(p);
        const TwPtr tw = as_global(INV ? p.inv : p.fwd);
        for (int tid = 0; tid < PASS::THREADS; tid++) PASS::template phase<0>(tid, base, lds.data(), tw, row0, ctx, p.inv_n);
        if constexpr (PASS::NPHASE > 1)
            for (int tid = 0; tid < PASS::THREADS; tid++) PASS::template phase<1>(tid, base, lds.data(), tw, row0, ctx, p.inv_n);
        if constexpr (PASS::NPHASE > 2)
            for (int tid = 0; tid < PASS::THREADS; tid++) PASS::template phase<2>(tid, base, lds.data(), tw, row0, ctx, p.inv_n);
        if constexpr (PASS::NPHASE > 3)
            for (int tid = 0; tid < PASS::THREADS; tid++) PASS::template phase<3>(tid, base, lds.data(), tw, row0, ctx, p.inv_n);
        if constexpr (PASS::NPHASE > 4)
            for (int tid = 0; tid < PASS::THREADS; tid++) PASS::template phase<4>(tid, base, lds.data(), tw, row0, ctx, p.inv_n);
    }
}

template <class A, int LOGN, bool INV>
void emu_transform(const PassArgs &a)
{
    typedef Passes<A, LOGN, INV, (LOGN >= 13 ? 1 : 0)> PS;   // the geometry launch_ntt uses by default
    if constexpr (!PS::G::TWO_PASS) {
        emu_pass<typename PS::Single, LOGN, INV, false>(a);
    } else if constexpr (!INV) {
        emu_pass<typename PS::Col, LOGN, INV, true>(a);
        emu_pass<typename PS::Row, LOGN, INV, false>(a);
    } else {
        emu_pass<typename PS::Row, LOGN, INV, false>(a);
        emu_pass<typename PS::Col, LOGN, INV, true>(a);
    }
}

// forward transform with the packed hand-off (ntt_core.hpp): the kernels' phase order with the per-thread registers that
// live across a barrier (chunk / x) kept per thread id
template <class A, int LOGN>
int emu_packed(const PassArgs &a)
{
    typedef Passes<A, LOGN, false, 1> PS;
    typedef typename PS::Col CP;
    typedef typename PS::Row RP;
    if constexpr (PS::G::TWO_PASS && A::PATH == PATH_F64) {
        if constexpr (CP::PACKABLE && RP::PACKABLE) {
            std::vector<u64> scratch((size_t)a.units * 256 * PK_BLOCK_WORDS, 0xDEADBEEFDEADBEEFull);
            std::vector<typename A::elem> lds(cmax(CP::LDS_ELEMS, RP::LDS_ELEMS));
            u64 *stage = reinterpret_cast<u64 *>(lds.data());
            for (u32 b = 0; b < a.units * CP::TILES; b++) {
                u32 limb;
                u64 *base = col_tile<CP, LOGN>(b, a, limb);
                const u32 unit = b / CP::TILES, tile = b % CP::TILES;
                const LimbParams &p = a.lp[limb];
                auto ctx = A::make_ctx(p);
                const TwPtr tw = as_global(p.fwd);
                for (int tid = 0; tid < CP::THREADS; tid++) CP::template phase<0>(tid, base, lds.data(), tw, 0u, ctx, p.inv_n);
                std::vector<std::array<u64, PK_WORDS>> chunk(CP::THREADS);
                for (int tid = 0; tid < CP::THREADS; tid++) {
                    u64 c[PK_WORDS];
                    CP::phase_last_packed(tid, lds.data(), tw, 0u, ctx, c);
                    for (int j = 0; j < PK_WORDS; j++) chunk[tid][j] = c[j];
                }
                for (int tid = 0; tid < CP::THREADS; tid++) {
                    u64 c[PK_WORDS];
                    for (int j = 0; j < PK_WORDS; j++) c[j] = chunk[tid][j];
                    CP::pack_stage(tid, stage, c);
                }
                for (int tid = 0; tid < CP::THREADS; tid++)
                    CP::pack_copy_out(tid, stage, scratch.data() + ((size_t)unit * 256 + (size_t)tile * 16) * PK_BLOCK_WORDS);
            }
            for (u32 b = 0; b < a.units * RP::TILES; b++) {
                u32 limb, row0 = 0;
                u64 *base = row_tile<RP, LOGN>(b, a, limb, row0);
                const u32 unit = b / RP::TILES, tile = b % RP::TILES;
                const LimbParams &p = a.lp[limb];
                auto ctx = A::make_ctx(p);
                const TwPtr tw = as_global(p.fwd);
                for (int tid = 0; tid < RP::THREADS; tid++) RP::unpack_copy_in(tid, stage, scratch.data() + (size_t)unit * 256 * PK_BLOCK_WORDS, tile);
                std::vector<std::array<typename A::elem, 16>> xs(RP::THREADS);
                for (int tid = 0; tid < RP::THREADS; tid++) {
                    typename A::elem x[16];
                    RP::phase_first_packed(tid, stage, tw, row0, ctx, x);
                    for (int r = 0; r < 16; r++) xs[tid][r] = x[r];
                }
                for (int tid = 0; tid < RP::THREADS; tid++) {
                    typename A::elem x[16];
                    for (int r = 0; r < 16; r++) x[r] = xs[tid][r];
                    RP::phase_first_store(tid, lds.data(), x);
                }
                for (int tid = 0; tid < RP::THREADS; tid++) RP::template phase<1>(tid, base, lds.data(), tw, row0, ctx, p.inv_n);
                for (int tid = 0; tid < RP::THREADS; tid++) RP::template phase<2>(tid, base, lds.data(), tw, row0, ctx, p.inv_n);
            }
            return 0;
        }
    }
    return -1;
}

// LDS-resident single pass of 2^13 / 2^14 (ntt_plan.hpp ResidentPlan)
template <class A, int LOGN>
int emu_resident(const PassArgs &a, int inverse)
{
    if constexpr (ResidentPlan<LOGN>::OK) {
        if (inverse) emu_pass<typename ResidentPass<A, LOGN, true>::Pass, LOGN, true, false>(a);
        else emu_pass<typename ResidentPass<A, LOGN, false>::Pass, LOGN, false, false>(a);
        return 0;
    }
    return -1;
}

template <class A, int LOGN>
void emu_dir(const PassArgs &a, int inverse)
{
    if (inverse) emu_transform<A, LOGN, true>(a);
    else emu_transform<A, LOGN, false>(a);
}

template <class A>
int emu_size(const PassArgs &a, int logn, int inverse)
{
    switch (logn) {
#define CASE(L) case L: emu_dir<A, L>(a, inverse); return 0;
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10)
        CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16) CASE(17) CASE(18) CASE(19) CASE(20)
#undef CASE
    default: return -1;
    }
}

// the fused kernel's ticket schedule, run by ONE sequential "team": every wait is already
// satisfied when its ticket comes up, which is exactly the progress argument of ntt_fused.hpp
template <class PASS, int LOGN, bool INV, bool IS_COL>
void emu_tile(const PassArgs &a, u32 unit, u32 tile, std::vector<typename PASS::elem> &lds)
{
    typedef typename PASS::Arith A;
    u32 limb, row0 = 0;
    u64 *base;
    if constexpr (IS_COL) base = col_tile_of<PASS, LOGN>(unit, tile, a, limb);
    else base = row_tile_of<PASS, LOGN>(unit, tile, a, limb, row0);
    const LimbParams &p = a.lp[limb];
    auto ctx = A::make_ctx(p);
    const TwPtr tw = as_global(INV ? p.inv : p.fwd);
    for (int tid = 0; tid < PASS::THREADS; tid++) PASS::template phase<0>(tid, base, lds.data(), tw, row0, ctx, p.inv_n);
    if constexpr (PASS::NPHASE > 1)
        for (int tid = 0; tid < PASS::THREADS; tid++) PASS::template phase<1>(tid, base, lds.data(), tw, row0, ctx, p.inv_n);
    if constexpr (PASS::NPHASE > 2)
        for (int tid = 0; tid < PASS::THREADS; tid++) PASS::template phase<2>(tid, base, lds.data(), tw, row0, ctx, p.inv_n);
    if constexpr (PASS::NPHASE > 3)
        for (int tid = 0; tid < PASS::THREADS; tid++) PASS::template phase<3>(tid, base, lds.data(), tw, row0, ctx, p.inv_n);
}

template <class A, int LOGN, bool INV>
int emu_fused(const PassArgs &a, u32 dist)
{
    typedef FusedPasses<A, LOGN, INV> FP;
    std::vector<typename A::elem> lds(FP::LDS_ELEMS);
    // teams run one after the other here; on the GPU they run concurrently and independently
    for (u32 x = 0; x < FUSED_TEAMS; x++) {
        const u32 my_limbs = fused_team_limbs(a.units, x), last_group = my_limbs + dist;
        std::vector<u32> done(my_limbs + 1, 0);
        for (u32 t = 0;; t++) {
            const FusedTicket k = fused_decode(t, FP::T1, FP::T2, dist);
            if (k.group >= last_group) break;
            if (k.phase == 0 || k.slot >= my_limbs) continue;
            const u32 unit = x + FUSED_TEAMS * k.slot;
            if (k.phase == 1) {
                if constexpr (INV) emu_tile<typename FP::Row, LOGN, INV, false>(a, unit, k.tile, lds);
                else emu_tile<typename FP::Col, LOGN, INV, true>(a, unit, k.tile, lds);
                done[k.slot]++;
            } else {
                if (done[k.slot] != FP::T1) return -4;   // a wait that would block: schedule bug
                if constexpr (INV) emu_tile<typename FP::Col, LOGN, INV, true>(a, unit, k.tile, lds);
                else emu_tile<typename FP::Row, LOGN, INV, false>(a, unit, k.tile, lds);
            }
        }
    }
    return 0;
}

template <class A>
int emu_fused_size(const PassArgs &a, int logn, int inverse, u32 dist)
{
    switch (logn) {
#define CASE(L) case L: return inverse ? emu_fused<A, L, true>(a, dist) : emu_fused<A, L, false>(a, dist);
        CASE(13) CASE(14) CASE(15) CASE(16) CASE(17)
#undef CASE
    default: return -1;
    }
}

// The two launches of the natural-order transform as launch_gs_t makes them (ntt_plan.hpp GsPasses): the gathering inverse row pass
// fed from the natural-order source, then the inverse column pass on the hand-off buffer; single-launch sizes are the first alone.
template <class PASS, int E = 0>
void gs_phases(u64 *base, typename PASS::elem *lds, TwPtr tw, u32 row0, const typename PASS::Arith::Ctx &ctx, const Tw &inv_n, const u64 *from)
{
    if constexpr (E < PASS::NPHASE) {
        for (int tid = 0; tid < PASS::THREADS; tid++) PASS::template phase<E>(tid, base, lds, tw, row0, ctx, inv_n, (NoTap *)nullptr, from);
        gs_phases<PASS, E + 1>(base, lds, tw, row0, ctx, inv_n, from);
    }
}

template <class A, int LOGN>
void emu_gs(u64 *dst, const u64 *src, const LimbParams &p)
{
    typedef GsPasses<A, LOGN> GP;
    typedef typename GP::First First;
    const auto ctx = A::make_ctx(p);
    const TwPtr tw = as_global(p.inv);
    std::vector<u64> tmp((size_t)1 << LOGN);
    u64 *first_out = GP::TWO ? tmp.data() : dst;
    {
        std::vector<typename First::elem> lds(First::LDS_ELEMS);
        for (u32 tile = 0; tile < (u32)First::TILES; tile++) gs_phases<First>(first_out, lds.data(), tw, tile * First::TROWS, ctx, p.inv_n, src);
    }
    if constexpr (GP::TWO) {
        typedef typename GP::Second Col;
        std::vector<typename Col::elem> lds(Col::LDS_ELEMS);
        PassArgs a{dst, &p, 0u, 1u, 1u, 1u};
        for (u32 b = 0; b < (u32)Col::TILES; b++) {
            u32 limb;
            u64 *base = col_tile<Col, LOGN>(b, a, limb);
            gs_phases<Col>(base, lds.data(), tw, 0u, ctx, p.inv_n, tmp.data() + (base - dst));
        }
    }
}

u64 invmod(u64 a, u64 m)
{
    __int128 t = 0, nt = 1, r = m, nr = a % m;
    while (nr != 0) {
        __int128 q = r / nr, tmp;
        tmp = t - q * nt; t = nt; nt = tmp;
        tmp = r - q * nr; r = nr; nr = tmp;
    }
    if (t < 0) t += m;
    return (u64)t;
}

} // namespace

// data: [n_poly][limbs][N] in place.  q: limbs moduli.  rp: limbs x N forward tables
// (canonical residues, entry k = psi^bitrev(k)).  path: 0 = ArithF64, 1 = ArithU64.
extern "C" int emu_ntt(u64 *data, int logn, int inverse, int n_poly, int limbs, const u64 *q, const u64 *rp, int path,
                       int fused_dist)
{
    const size_t N = (size_t)1 << logn;
    std::vector<LimbParams> lp(limbs);
    std::vector<std::vector<Tw>> fwd(limbs), inv(limbs);
    for (int l = 0; l < limbs; l++) {
        fwd[l].resize(N);
        inv[l].resize(N);
        for (size_t k = 0; k < N; k++) {
            u64 w = rp[(size_t)l * N + k], wi = invmod(w, q[l]);
            const u32 at = tw_stored_index(logn, (u32)k);   // same layout the library uploads
            fwd[l][at] = path == PATH_F64 ? ArithF64::encode(w, q[l]) : ArithU64::encode(w, q[l]);
            inv[l][at] = path == PATH_F64 ? ArithF64::encode(wi, q[l]) : ArithU64::encode(wi, q[l]);
        }
        {   // inverse entry 0: N^-1 times the last inverse stage's twiddle (as capi.cpp build_tables lays it out)
            const u64 ni0 = invmod(N % q[l], q[l]), w1 = invmod(rp[(size_t)l * N + (N > 1 ? 1 : 0)], q[l]);
            const u64 wn = (u64)((unsigned __int128)ni0 * w1 % q[l]);
            inv[l][0] = path == PATH_F64 ? ArithF64::encode(wn, q[l]) : ArithU64::encode(wn, q[l]);
        }
        LimbParams &p = lp[l];
        p.q = q[l];
        p.two_q = 2 * q[l];
        p.n = (double)q[l];
        p.ninv = 1.0 / p.n;
        u64 ni = invmod(N % q[l], q[l]);
        p.inv_n = path == PATH_F64 ? ArithF64::encode(ni, q[l]) : ArithU64::encode(ni, q[l]);
        p.fwd = fwd[l].data();
        p.inv = inv[l].data();
        p.path = path;
    }
    PassArgs a{data, lp.data(), 0u, (u32)limbs, (u32)(n_poly * limbs), (u32)limbs};
    // fused_dist == -1: the same batch addressed through an explicit unit list (PassArgs::map), in reverse order
    std::vector<UnitRef> map;
    if (fused_dist == -1) {
        for (int u = n_poly * limbs - 1; u >= 0; u--) map.push_back(UnitRef{(u32)u, (u32)(u % limbs)});
        a.map = map.data();
    }
    g_max_ratio = g_max_pair = 0.0;      // the maxima are per call
    for (u64 &e : g_ev) e = 0;            // and so are the integer path's events
    if (fused_dist == -3) {          // forward transform with the packed hand-off (2^16, FP64 path)
        if (logn == 16 && path == PATH_F64 && !inverse) return emu_packed<TrackF64, 16>(a);
        return -1;
    }
    if (fused_dist == -2) {          // resident pass
        if (logn == 13) return path == PATH_F64 ? emu_resident<TrackF64, 13>(a, inverse) : emu_resident<TrackU64, 13>(a, inverse);
        if (logn == 14) return path == PATH_F64 ? emu_resident<TrackF64, 14>(a, inverse) : emu_resident<TrackU64, 14>(a, inverse);
        return -1;
    }
    if (fused_dist > 0)
        return path == PATH_F64 ? emu_fused_size<TrackF64>(a, logn, inverse, (u32)fused_dist)
                                : emu_fused_size<TrackU64>(a, logn, inverse, (u32)fused_dist);
    return path == PATH_F64 ? emu_size<TrackF64>(a, logn, inverse) : emu_size<TrackU64>(a, logn, inverse);
}

// Natural-order transform of one vector under the tracker (FP64 path, q < 2^50): dst = scale * W src, src and dst in natural order
// (dst may equal src).  tw: the cyclic table in canonical residues, tw[2^s + bitrev(k, s)] = w_s^k, laid out and scaled as capi.cpp
// build_tables does with gs_scale: entry 0 = scale * tw[1], inv_n = scale.
extern "C" int emu_ntt_gs(u64 *dst, const u64 *src, int logn, u64 q, const u64 *tw, u64 scale)
{
    if (logn < 5 || logn > 20 || q < 2 || q >= ((u64)1 << 50)) return -1;
    const size_t N = (size_t)1 << logn;
    std::vector<Tw> inv(N);
    for (size_t k = 1; k < N; k++) inv[tw_stored_index(logn, (u32)k)] = ArithF64::encode(tw[k] % q, q);
    inv[0] = ArithF64::encode((u64)((unsigned __int128)(scale % q) * (tw[1] % q) % q), q);
    LimbParams p{};
    p.q = q;
    p.two_q = 2 * q;
    p.n = (double)q;
    p.ninv = 1.0 / p.n;
    p.inv_n = ArithF64::encode(scale % q, q);
    p.fwd = inv.data();
    p.inv = inv.data();
    p.path = PATH_F64;
    g_max_ratio = g_max_pair = 0.0;
    switch (logn) {
#define CASE(L) case L: emu_gs<TrackF64, L>(dst, src, p); return 0;
        CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16) CASE(17) CASE(18) CASE(19) CASE(20)
#undef CASE
    default: return -1;
    }
}

// maxima of the last emu_ntt / emu_ntt_gs call (path 0; the integer path leaves them 0): register values, and inverse pair sums
extern "C" double emu_max_ratio() { return g_max_ratio; }
extern "C" double emu_max_pair() { return g_max_pair; }
// events of the last emu_ntt call on path 1 and of the emu_u64_mulvar_lazy calls since (the FP64 path leaves them 0), in the order of
// the EV_ enumeration: X == 2q at the forward fold, X + Y == 2q at the inverse sum, a word q / 2q / 3q on entry to canonical(), a
// Shoup product in [q, 2q), barrett128 left exactly q before its first fix-up, an operand outside its documented range
extern "C" void emu_u64_events(u64 *out)
{
    for (int i = 0; i < EV_COUNT; i++) out[i] = g_ev[i];
}
// c[i] = ArithU64::mulvar_lazy(a[i], b[i]) under the tracker: the one Barrett step of the fused product, on lazy words
extern "C" void emu_u64_mulvar_lazy(u64 *c, const u64 *a, const u64 *b, size_t n, u64 q)
{
    LimbParams p{};
    p.q = q;
    p.two_q = 2 * q;
    const unsigned __int128 ratio = ~(unsigned __int128)0 / q;      // = floor(2^128 / q): q is odd, so it does not divide 2^128
    p.barrett_lo = (u64)ratio;
    p.barrett_hi = (u64)(ratio >> 64);
    for (size_t i = 0; i < n; i++) c[i] = TrackU64::mulvar_lazy(a[i], b[i], p);
}

// the per-register lazy-range plan of K inverse stages (ntt_core.hpp inv_lazy_plan), as the kernels' templates evaluate it
template <int K> static void dump_plan(int in8, int exit8, int fold, uint32_t *before, uint32_t *at_exit, int *out8)
{
    const InvLazyPlan<K> p = inv_lazy_plan<K>(in8, exit8, fold != 0);
    for (int v = 0; v < K; v++) before[v] = p.before[v];
    *at_exit = p.at_exit;
    *out8 = p.out8;
}
extern "C" int emu_inv_lazy_plan(int K, int in8, int exit8, int fold, uint32_t *before, uint32_t *at_exit, int *out8)
{
    switch (K) {
    case 1: dump_plan<1>(in8, exit8, fold, before, at_exit, out8); return 0;
    case 2: dump_plan<2>(in8, exit8, fold, before, at_exit, out8); return 0;
    case 3: dump_plan<3>(in8, exit8, fold, before, at_exit, out8); return 0;
    case 4: dump_plan<4>(in8, exit8, fold, before, at_exit, out8); return 0;
    case 5: dump_plan<5>(in8, exit8, fold, before, at_exit, out8); return 0;
    default: return 1;
    }
}
// entry bound of the second launch of a two-launch inverse and of every step, as Passes<> derives them (2^16: Steps<4,4> twice)
extern "C" int emu_inv_lazy_chain(int k0, int k1, int k2, int in8, int se)
{
    if (k2) return k1 == 3 ? inv_lazy_step_in8<Steps<3, 3, 3>>(in8, se) : inv_lazy_step_in8<Steps<4, 4, 4>>(in8, se);
    if (k0 == 4 && k1 == 4) return inv_lazy_step_in8<Steps<4, 4, 0>>(in8, se);
    if (k0 == 4 && k1 == 3) return inv_lazy_step_in8<Steps<4, 3, 0>>(in8, se);
    return -1;
}

// ---------------------------------------------------------------------------
// The fold schedule of every pass as its template arguments fix it, for the exact-fraction walks of tests/test_ntt_worst_case.py.
// A pass writes 6 ints { kind (0 row, 1 column), steps, input mode, output mode, lazy inverse plan?, its declared entry bound in
// eighths of q } and then 5 ints per register step in execution order { K, fold mask of its K stages (bit v = before executed
// stage v; -1 under the per-register plan), entry bound and exit bound in eighths of q (per-register plan), N^-1 folded into
// the last stage? }.  The step formulas are those of ColPass::phase / RowPass::phase.
// ---------------------------------------------------------------------------
namespace {

struct SchedOut {
    int *out, cap, n;
    void put(int v)
    {
        if (n < cap) out[n] = v;
        n++;
    }
};

template <class A, class ST, int S0, bool INV, int IN_MODE, int OUT_MODE, u32 RED, int... SE>
void sched_steps(SchedOut &o, int kind, int in_mode, int out_mode, std::integer_sequence<int, SE...>)
{
    constexpr bool LAZY = INV && (RED & INV_LAZY) != 0 && A::PATH == PATH_F64;
    o.put(kind), o.put(ST::NSTEP), o.put(in_mode), o.put(out_mode), o.put(LAZY), o.put(LAZY ? (int)(RED & 0xFFu) : 0);
    auto step = [&](auto se_c) {
        constexpr int E = decltype(se_c)::value;
        constexpr int F = INV ? ST::NSTEP - 1 - E : E, K = ST::k(F), DONE = ST::done(F);
        constexpr int U0 = INV ? (ST::P - DONE - K) : DONE;
        constexpr bool LAST = E == ST::NSTEP - 1;
        constexpr bool FOLD = INV && LAST && OUT_MODE == IO_CANONICAL && S0 + DONE == 0;
        o.put(K);
        o.put(LAZY ? -1 : (int)((RED >> U0) & ((1u << K) - 1u)));
        o.put(LAZY ? inv_lazy_step_in8<ST>((int)(RED & 0xFFu), E) : 0);
        o.put(LAZY ? ((LAST && OUT_MODE == IO_CANONICAL) ? INV_LAZY_LIMIT8 : INV_LAZY_EXIT8) : 0);
        o.put(FOLD);
    };
    (step(std::integral_constant<int, SE>{}), ...);
}

template <class T> struct PassInfo;
template <class A, class ST, int LOGN, int TR, int NT, bool INV, int IN_MODE, int OUT_MODE, u32 RED, int SBLK, int CO, bool STREAM, bool SBOTH, int RM>
struct PassInfo<RowPass<A, ST, LOGN, TR, NT, INV, IN_MODE, OUT_MODE, RED, SBLK, CO, STREAM, SBOTH, RM>> {
    static void dump(SchedOut &o, int in_mode = IN_MODE, int out_mode = OUT_MODE)
    {
        sched_steps<A, ST, LOGN - ST::P, INV, IN_MODE, OUT_MODE, RED>(o, 0, in_mode, out_mode, std::make_integer_sequence<int, ST::NSTEP>{});
    }
};
template <class A, class ST, int LOGN, int S0, int TC, int NT, bool INV, int IN_MODE, int OUT_MODE, u32 RED, int SBLK, int CO, bool STREAM>
struct PassInfo<ColPass<A, ST, LOGN, S0, TC, NT, INV, IN_MODE, OUT_MODE, RED, SBLK, CO, STREAM>> {
    static void dump(SchedOut &o, int in_mode = IN_MODE, int out_mode = OUT_MODE)
    {
        sched_steps<A, ST, S0, INV, IN_MODE, OUT_MODE, RED>(o, 1, in_mode, out_mode, std::make_integer_sequence<int, ST::NSTEP>{});
    }
};

// form 0: Passes (both launches), 1: FusedPasses, 2: ResidentPass, 3: MidPasses (forward row pass, then inverse row pass),
// 4: Passes forward with the packed hand-off (canonical residues between the launches),
// 5: GsPasses, the natural-order route (inverse network only, 2^5 and up): the gathering first launch, then the column pass
template <int LOGN, bool INV> int sched_form(SchedOut &o, int form)
{
    typedef ArithF64 A;
    constexpr int GEO = LOGN >= 13 ? 1 : 0;
    typedef Passes<A, LOGN, INV, GEO> PS;
    if (form == 0) {
        if constexpr (!PS::G::TWO_PASS) PassInfo<typename PS::Single>::dump(o);
        else if constexpr (!INV) PassInfo<typename PS::Col>::dump(o), PassInfo<typename PS::Row>::dump(o);
        else PassInfo<typename PS::Row>::dump(o), PassInfo<typename PS::Col>::dump(o);
        return 0;
    }
    if (form == 1) {
        if constexpr (LOGN >= 13 && LOGN <= 17) {
            typedef FusedPasses<A, LOGN, INV> FP;
            if constexpr (!INV) PassInfo<typename FP::Col>::dump(o), PassInfo<typename FP::Row>::dump(o);
            else PassInfo<typename FP::Row>::dump(o), PassInfo<typename FP::Col>::dump(o);
            return 0;
        }
        return -1;
    }
    if (form == 2) {
        if constexpr (ResidentPlan<LOGN>::OK) {
            PassInfo<typename ResidentPass<A, LOGN, INV>::Pass>::dump(o);
            return 0;
        }
        return -1;
    }
    if (form == 3) {
        typedef MidPasses<A, LOGN, GEO> MP;
        if constexpr (!INV) PassInfo<typename MP::Fwd>::dump(o);
        else PassInfo<typename MP::Inv>::dump(o);
        return 0;
    }
    if (form == 4) {
        if constexpr (LOGN == 16 && !INV) {
            PassInfo<typename PS::Col>::dump(o, IO_CANONICAL, IO_CANONICAL);
            PassInfo<typename PS::Row>::dump(o, IO_CANONICAL, IO_CANONICAL);
            return 0;
        }
        return -1;
    }
    if (form == 5) {
        if constexpr (INV && LOGN >= 5) {
            typedef GsPasses<A, LOGN> GP;
            PassInfo<typename GP::First>::dump(o);
            if constexpr (GP::TWO) PassInfo<typename GP::Second>::dump(o);
            return 0;
        }
        return -1;
    }
    return -1;
}

} // namespace

// returns the number of ints the schedule takes (written up to cap), or a negative value where the form does not exist at that size
extern "C" int emu_fold_schedule(int form, int logn, int inverse, int *out, int cap)
{
    SchedOut o{out, cap, 0};
    int rc = -1;
    switch (logn) {
#define CASE(L) case L: rc = inverse ? sched_form<L, true>(o, form) : sched_form<L, false>(o, form); break;
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10)
        CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16) CASE(17) CASE(18) CASE(19) CASE(20)
#undef CASE
    default: break;
    }
    return rc < 0 ? rc : o.n;
}
// the stage budgets the masks above were built from
extern "C" void emu_f64_budgets(int *b)
{
    b[0] = ArithF64::FWD_FIRST, b[1] = ArithF64::FWD_NEXT, b[2] = ArithF64::INV_FIRST, b[3] = ArithF64::INV_NEXT;
}
