// emu_ntt_seal.cpp -- CPU emulation of the sealed inverse transform's first launch (TEST INFRASTRUCTURE ONLY).
//
// Compiles fhe_reliability_gpu_amd/csrc/ntt_seal_tap.hpp together with ntt_core.hpp / ntt_plan.hpp with g++ and runs the first
// launch of the checked inverse (the inverse row pass of the two-launch sizes, the single pass below 2^13) tile by tile, thread by
// thread, with the very pass templates and the very tap k_ntt_pass_sealed_io instantiates (SealPassTap) -- out of place from a
// source array, so that the digest, the window, the hook and the words can be checked without a GPU.  emu_launch, one sealed launch
// of either direction, serves emu_ntt_fwd_seal.cpp as well.  The library never links this file.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I<csrc> emu_ntt_seal.cpp -o libemu_ntt_seal.so
#include "ntt_plan.hpp"
#include "ntt_seal_tap.hpp"

#include <type_traits>
#include <vector>

using namespace fhe;

namespace {

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

// the tables and limb constants of one limb, laid out as the library uploads them (capi.cpp build_tables)
struct Limb {
    LimbParams p;
    std::vector<Tw> fwd, inv, win, wout;
    std::vector<u64> wout8;
    Limb(int logn, u64 q, const u64 *rp, const u64 *w_hat, int path)
    {
        const size_t N = (size_t)1 << logn;
        auto enc = [&](u64 w) { return path == PATH_F64 ? ArithF64::encode(w, q) : ArithU64::encode(w, q); };
        fwd.resize(N);
        inv.resize(N);
        // the table's inverses by one invmod (prefix products, inverted once and peeled back): 2^20 entries in milliseconds
        auto mul = [&](u64 a, u64 b) { return (u64)((unsigned __int128)a * b % q); };
        std::vector<u64> pre(N), rinv(N);
        u64 acc = 1;
        for (size_t k = 0; k < N; k++) {
            pre[k] = acc;
            acc = mul(acc, rp[k]);
        }
        u64 ia = invmod(acc, q);
        for (size_t k = N; k-- > 0;) {
            rinv[k] = mul(ia, pre[k]);
            ia = mul(ia, rp[k]);
        }
        for (size_t k = 0; k < N; k++) {
            const u32 at = tw_stored_index(logn, (u32)k);
            fwd[at] = enc(rp[k]);
            inv[at] = enc(rinv[k]);
        }
        const u64 ni = invmod(N % q, q);
        inv[0] = enc((u64)((unsigned __int128)ni * invmod(rp[N > 1 ? 1 : 0], q) % q));
        const u64 p2 = (u64)1 << (logn / 2);
        win.resize(N);
        wout.resize(N);
        wout8.assign(w_hat, w_hat + N);
        for (size_t i = 0; i < N; i++) {
            win[i] = enc(((i % p2 + 1) + (i / p2 + 1)) % q);
            wout[i] = enc(w_hat[i]);
        }
        p.q = q;
        p.two_q = 2 * q;
        p.n = (double)q;
        p.ninv = 1.0 / p.n;
        const unsigned __int128 ratio = ~(unsigned __int128)0 / q;     // floor(2^128 / q), q odd
        p.barrett_lo = (u64)ratio;
        p.barrett_hi = (u64)(ratio >> 64);
        p.inv_n = enc(ni);
        p.fwd = fwd.data();
        p.inv = inv.data();
        p.path = path;
    }
};

// every phase of one tile, thread by thread, loading from `from`
template <class PASS, class TAP>
void run_tile(u64 *base, const u64 *from, typename PASS::elem *lds, TwPtr tw, u32 row0, const typename PASS::Arith::Ctx &ctx, const Tw &inv_n, TAP *t)
{
    auto run = [&](auto e) {
        constexpr int E = decltype(e)::value;
        if constexpr (E < PASS::NPHASE) {
            for (int tid = 0; tid < PASS::THREADS; tid++) PASS::template phase<E>(tid, base, lds, tw, row0, ctx, inv_n, t, from);
        }
    };
    run(std::integral_constant<int, 0>());
    run(std::integral_constant<int, 1>());
    run(std::integral_constant<int, 2>());
    run(std::integral_constant<int, 3>());
    run(std::integral_constant<int, 4>());
}

struct IoOut {
    u64 *parts_in, *parts_out, *sums;      // [tin][3], [tout][2], {sum_in, sum_out}
    int tin, tout;
};

// one sealed launch: every tile of PASS over dst (loading from src where IN) with the tap k_ntt_pass_sealed_io builds (hooked when
// hit_coeff >= 0), the tiles' partials and ABFT sums collected.  The one place where the tap is constructed and read back
template <class PASS, int LOGN, bool IS_COL, bool INV, bool IN, bool OUT, bool DIGEST = OUT>
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
            const u32 hit_idx = HOOK ? ntt_seal_tile_hit<PASS, IS_COL>((u32)hit_coeff, pos0) : NTT_SEAL_NO_HIT;
            SealPassTap<A, INV, HOOK, IN, OUT, DIGEST> tap{
                {L.win.data() + pos0, L.wout.data() + pos0, L.wout8.data() + pos0, pos0, LOGN / 2, typename A::elem(0), typename A::elem(0), 0, 0},
                SealAcc{}, 0u, L.p.q, hit_idx, (u64)1 << hit_bit, SealAcc{}};
            run_tile<PASS>(base, from, lds.data(), tw, row0, ctx, L.p.inv_n, &tap);
            if constexpr (IN) {
                o.sums[0] = (o.sums[0] + A::canonical(tap.acc_in, ctx)) % L.p.q;
                o.parts_in[NTT_SEAL_PART * b] = tap.seal.s0;
                o.parts_in[NTT_SEAL_PART * b + 1] = tap.seal.s1;
                o.parts_in[NTT_SEAL_PART * b + 2] = tap.n_range;
                o.tin = (int)PASS::TILES;
            }
            if constexpr (OUT) o.sums[1] = (o.sums[1] + A::canonical(tap.acc_out, ctx)) % L.p.q;
            if constexpr (DIGEST) {
                o.parts_out[NTT_SEAL_OUT_PART * b] = tap.seal_out.s0;
                o.parts_out[NTT_SEAL_OUT_PART * b + 1] = tap.seal_out.s1;
                o.tout = (int)PASS::TILES;
            }
        };
        if (IN && hit_coeff >= 0) tapped(std::bool_constant<IN>());
        else tapped(std::false_type());
    }
}

// mode 0: no tap; 1: the sealed first launch, through emu_launch; 2: InvChecksumTap (the checked inverse's own first launch)
template <class PASS, int LOGN, bool OUT>
int emu_first(const u64 *src, u64 *dst, const Limb &L, int mode, long long hit_coeff, int hit_bit, u64 *parts, u64 *sum_in)
{
    typedef typename PASS::Arith A;
    *sum_in = 0;
    if (mode == 1) {      // the single pass forms the output-side ABFT sum and no output digest
        u64 sums[2] = {0, 0};
        IoOut o{parts, nullptr, sums, 0, 0};
        emu_launch<PASS, LOGN, false, true, true, OUT, false>(src, dst, L, hit_coeff, hit_bit, o);
        *sum_in = sums[0];
        return o.tin;
    }
    PassArgs a{dst, &L.p, 0u, 1u, 1u, 1u};
    std::vector<typename PASS::elem> lds(PASS::LDS_ELEMS > 0 ? PASS::LDS_ELEMS : 1);
    const auto ctx = A::make_ctx(L.p);
    const TwPtr tw = as_global(L.p.inv);
    for (u32 b = 0; b < PASS::TILES; b++) {
        u32 limb, row0 = 0;
        u64 *base = row_tile<PASS, LOGN>(b, a, limb, row0);
        const u32 pos0 = (u32)(base - dst);
        const u64 *from = src + pos0;
        if (mode == 0) {
            run_tile<PASS, NoTap>(base, from, lds.data(), tw, row0, ctx, L.p.inv_n, nullptr);
        } else {
            InvChecksumTap<A, true, OUT> tap{L.win.data() + pos0, L.wout.data() + pos0, L.wout8.data() + pos0, pos0, LOGN / 2, typename A::elem(0), typename A::elem(0), 0, 0};
            run_tile<PASS>(base, from, lds.data(), tw, row0, ctx, L.p.inv_n, &tap);
            *sum_in = (*sum_in + A::canonical(tap.acc_in, ctx)) % L.p.q;
        }
    }
    return (int)PASS::TILES;
}

template <class A, int LOGN>
int emu_size(const u64 *src, u64 *dst, const Limb &L, int mode, long long hit_coeff, int hit_bit, u64 *parts, u64 *sum_in)
{
    typedef Passes<A, LOGN, true, (LOGN >= 13 ? 1 : 0)> PS;
    if constexpr (!PS::G::TWO_PASS) return emu_first<typename PS::Single, LOGN, true>(src, dst, L, mode, hit_coeff, hit_bit, parts, sum_in);
    else return emu_first<typename PS::Row, LOGN, false>(src, dst, L, mode, hit_coeff, hit_bit, parts, sum_in);
}

template <class A>
int dispatch(int logn, const u64 *src, u64 *dst, const Limb &L, int mode, long long hit_coeff, int hit_bit, u64 *parts, u64 *sum_in)
{
    switch (logn) {
#define CASE(LG) case LG: return emu_size<A, LG>(src, dst, L, mode, hit_coeff, hit_bit, parts, sum_in);
        CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16) CASE(17) CASE(18) CASE(19) CASE(20)
#undef CASE
    default: return -1;
    }
}

} // namespace

// The first launch of the checked inverse of one limb-polynomial, out of place from src into dst (the lazy words it hands to the
// column pass; below 2^13 the transform's final words).  Returns the number of tiles (parts = [tiles][3] lazily reduced {S0, S1,
// n_range}, mode 1 only), or -1.  rp = forward table (entry k = psi^bitrev(k)), w_hat = the ABFT input-side weights as residues.
extern "C" int emu_ntt_seal_first(const u64 *src, u64 *dst, int logn, u64 q, const u64 *rp, const u64 *w_hat, int path, int mode, long long hit_coeff, int hit_bit,
                                  u64 *parts, u64 *sum_in)
{
    const Limb L(logn, q, rp, w_hat, path);
    return path == PATH_F64 ? dispatch<ArithF64>(logn, src, dst, L, mode, hit_coeff, hit_bit, parts, sum_in)
                            : dispatch<ArithU64>(logn, src, dst, L, mode, hit_coeff, hit_bit, parts, sum_in);
}

// k_ntt_seal_finish for one row: the tiles' partials merged in the order given, made canonical into got[2], and the verdict
// against `stored` (may be null)
extern "C" unsigned emu_ntt_seal_finish(const u64 *parts, int tiles, const int *order, const u64 *stored, u64 *got)
{
    SealAcc acc;
    u64 nr = 0;
    for (int i = 0; i < tiles; i++) {
        const u64 *p = parts + (size_t)NTT_SEAL_PART * order[i];
        acc.merge(p[0], p[1]);
        nr += p[2];
    }
    got[0] = seal_canonical(acc.s0);
    got[1] = seal_canonical(acc.s1);
    return ntt_seal_verdict(acc, nr, stored);
}
