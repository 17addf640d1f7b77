// emu_ntt_fwd_seal.cpp -- CPU emulation of the sealed forward transform and of the sealed inverse with an output seal (TEST
// INFRASTRUCTURE ONLY).
//
// Runs every launch of the transform tile by tile, thread by thread, with SealFwdTap / SealInvTap (ntt_seal_tap.hpp) on the very
// pass templates k_ntt_pass_sealed_io instantiates: the launch that loads the input out of place from a source array with the input
// digest (and the hook), the launch that stores the result with the output digest; below 2^13 one pass with both.  The limb's tables
// and the tile runner are emu_ntt_seal.cpp's, included as they are.  The library never links this file.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I<csrc> emu_ntt_fwd_seal.cpp -o libemu_ntt_fwd_seal.so
#include "emu_ntt_seal.cpp"

namespace {

struct IoOut {
    u64 *parts_in, *parts_out, *sums;      // [tin][3], [tout][2], {sum_in, sum_out}
    int tin, tout;
};

// one launch: every tile of PASS over dst (loading from src where IN), the tiles' partials and ABFT sums collected
template <class PASS, int LOGN, bool IS_COL, bool INV, bool IN, bool OUT>
void emu_launch(const u64 *src, u64 *dst, const Limb &L, long long hit_coeff, int hit_bit, IoOut &o)
{
    typedef typename PASS::Arith A;
    PassArgs a{dst, &L.p, 0u, 1u, 1u, 1u};
    std::vector<typename PASS::elem> lds(PASS::LDS_ELEMS > 0 ? PASS::LDS_ELEMS : 1);
    const auto ctx = A::make_ctx(L.p);
    const TwPtr tw = as_global(INV ? L.p.inv : L.p.fwd);
    for (u32 b = 0; b < PASS::TILES; b++) {
        u32 limb, row0 = 0;
        u64 *base;
        if constexpr (IS_COL) base = col_tile<PASS, LOGN>(b, a, limb);
        else base = row_tile<PASS, LOGN>(b, a, limb, row0);
        const u32 pos0 = (u32)(base - dst);
        const u64 *from = IN && src != dst ? src + pos0 : nullptr;
        auto tapped = [&](auto hook) {
            constexpr bool HOOK = decltype(hook)::value;
            typedef std::conditional_t<INV, SealInvTap<A, HOOK, IN, OUT>, SealFwdTap<A, HOOK, IN, OUT>> Tap;
            const u32 hit_idx = HOOK ? ntt_seal_tile_hit<PASS, IS_COL>((u32)hit_coeff, pos0) : NTT_SEAL_NO_HIT;
            Tap tap{{L.win.data() + pos0, L.wout.data() + pos0, L.wout8.data() + pos0, pos0, LOGN / 2, typename A::elem(0), typename A::elem(0), 0, 0},
                    SealAcc{}, 0u, L.p.q, hit_idx, (u64)1 << hit_bit, SealAcc{}};
            run_tile<PASS>(base, from, lds.data(), tw, row0, ctx, L.p.inv_n, &tap);
            if constexpr (IN) {
                o.sums[0] = (o.sums[0] + A::canonical(tap.acc_in, ctx)) % L.p.q;
                o.parts_in[NTT_SEAL_PART * b] = tap.seal.s0;
                o.parts_in[NTT_SEAL_PART * b + 1] = tap.seal.s1;
                o.parts_in[NTT_SEAL_PART * b + 2] = tap.n_range;
                o.tin = (int)PASS::TILES;
            }
            if constexpr (OUT) {
                o.sums[1] = (o.sums[1] + A::canonical(tap.acc_out, ctx)) % L.p.q;
                o.parts_out[NTT_SEAL_OUT_PART * b] = tap.seal_out.s0;
                o.parts_out[NTT_SEAL_OUT_PART * b + 1] = tap.seal_out.s1;
                o.tout = (int)PASS::TILES;
            }
        };
        if (IN && hit_coeff >= 0) tapped(std::bool_constant<IN>());
        else tapped(std::false_type());
    }
}

template <class A, int LOGN, bool INV>
void emu_transform(const u64 *src, u64 *dst, const Limb &L, long long hit_coeff, int hit_bit, IoOut &o)
{
    typedef Passes<A, LOGN, INV, (LOGN >= 13 ? 1 : 0)> PS;
    if constexpr (!PS::G::TWO_PASS) {
        emu_launch<typename PS::Single, LOGN, false, INV, true, true>(src, dst, L, hit_coeff, hit_bit, o);
    } else if constexpr (INV) {
        emu_launch<typename PS::Row, LOGN, false, true, true, false>(src, dst, L, hit_coeff, hit_bit, o);
        emu_launch<typename PS::Col, LOGN, true, true, false, true>(dst, dst, L, -1, 0, o);
    } else {
        emu_launch<typename PS::Col, LOGN, true, false, true, false>(src, dst, L, hit_coeff, hit_bit, o);
        emu_launch<typename PS::Row, LOGN, false, false, false, true>(dst, dst, L, -1, 0, o);
    }
}

template <class A>
int dispatch_io(int logn, bool inverse, const u64 *src, u64 *dst, const Limb &L, long long hit_coeff, int hit_bit, IoOut &o)
{
    switch (logn) {
#define CASE(LG)                                                                 \
    case LG:                                                                     \
        if (inverse) emu_transform<A, LG, true>(src, dst, L, hit_coeff, hit_bit, o); \
        else emu_transform<A, LG, false>(src, dst, L, hit_coeff, hit_bit, o);    \
        return 0;
        CASE(5) CASE(12) CASE(13) CASE(14)
#undef CASE
    default: return -1;
    }
}

} // namespace

// The sealed transform of one limb-polynomial, out of place from src into dst.  parts_in = [tin][3] lazily reduced {S0, S1, n_range}
// of the loading launch, parts_out = [tout][2] lazily reduced {S0, S1} of the storing launch, sums = {ABFT sum_in, sum_out},
// tiles = {tin, tout}.  rp = forward table (entry k = psi^bitrev(k)), w_hat = the ABFT weights of the transformed side as residues.
// Returns 0, or -1 for a size the emulation is not instantiated for.
extern "C" int emu_ntt_sealed_io(int inverse, const u64 *src, u64 *dst, int logn, u64 q, const u64 *rp, const u64 *w_hat, int path, long long hit_coeff, int hit_bit,
                                 u64 *parts_in, u64 *parts_out, u64 *sums, int *tiles)
{
    const Limb L(logn, q, rp, w_hat, path);
    IoOut o{parts_in, parts_out, sums, 0, 0};
    sums[0] = sums[1] = 0;
    const int rc = path == PATH_F64 ? dispatch_io<ArithF64>(logn, inverse != 0, src, dst, L, hit_coeff, hit_bit, o)
                                    : dispatch_io<ArithU64>(logn, inverse != 0, src, dst, L, hit_coeff, hit_bit, o);
    tiles[0] = o.tin;
    tiles[1] = o.tout;
    return rc;
}

// k_ntt_seal_out_finish for one row: the tiles' output partials merged in the order given, then the poison rule
extern "C" void emu_ntt_seal_out_finish(const u64 *parts_out, int tiles, const int *order, unsigned flag_in, unsigned flag_abft, u64 *seal)
{
    SealAcc acc;
    for (int i = 0; i < tiles; i++) acc.merge(parts_out[(size_t)NTT_SEAL_OUT_PART * order[i]], parts_out[(size_t)NTT_SEAL_OUT_PART * order[i] + 1]);
    ntt_seal_out(acc, flag_in, flag_abft, seal);
}

// seal_differs (seal_check.hpp): what every verifier decides for lazily reduced digests (s0, s1) against a stored pair
extern "C" int emu_seal_differs(u64 s0, u64 s1, const u64 *stored) { return seal_differs(s0, s1, stored) ? 1 : 0; }
