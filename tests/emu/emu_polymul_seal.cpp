// emu_polymul_seal.cpp -- CPU emulation of the single-launch sealed negacyclic product (TEST INFRASTRUCTURE ONLY).
//
// Compiles fhe_reliability_gpu_amd/csrc/polymul_seal.hpp with g++ and runs the steps of PolymulSealMid -- the body of
// k_polymul_mid_sealed cut at its barriers -- one step at a time for every thread in turn, with the very taps and the very pass
// templates the kernel instantiates.  The limb's tables (Limb) are emu_ntt_seal.cpp's, included as it is.  The library never links
// this file.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I<csrc> emu_polymul_seal.cpp -o libemu_polymul_seal.so
#include "emu_ntt_seal.cpp"
#include "polymul_seal.hpp"

namespace {

// step S .. NSTEPS - 1, each for all threads before the next (the barrier between two steps)
template <class M, int S = 0>
void run_steps(const typename M::Tile &t, const typename M::FR::Arith::Ctx &ctx, std::vector<typename M::Lane> &lanes)
{
    if constexpr (S < M::NSTEPS) {
        for (int tid = 0; tid < NTT_THREADS; tid++) M::template step<S>(tid, t, ctx, lanes[tid]);
        run_steps<M, S + 1>(t, ctx, lanes);
    }
}

template <class A, int LOGN, bool HOOK>
void emu_mid(u64 *a, u64 *b, u64 *c, const Limb &L, int hit_op, long long hit_coeff, int hit_bit, u64 *parts, u64 *sums)
{
    typedef PolymulSealMid<A, LOGN, 0, true, HOOK> M;
    static_assert(M::FR::TILES == 1, "one tile per row below 2^13");
    std::vector<typename M::elem> lds(M::FR::LDS_ELEMS);
    const auto ctx = A::make_ctx(L.p);
    const u32 hit = HOOK ? ntt_seal_tile_hit<typename M::FR, false>((u32)hit_coeff, 0u) : NTT_SEAL_NO_HIT;
    const typename M::Tile t{a, b, c, lds.data(), &L.p, L.p.inv_n, 0u, L.wout.data(), L.wout8.data(), -1, 0};
    std::vector<typename M::Lane> lanes(NTT_THREADS, M::lane(L.win.data(), L.wout.data(), L.wout8.data(), 0u, LOGN / 2, L.p.q, hit_op == 0 ? hit : NTT_SEAL_NO_HIT,
                                                             hit_op == 1 ? hit : NTT_SEAL_NO_HIT, (u64)1 << hit_bit));
    run_steps<M>(t, ctx, lanes);
    SealAcc da, db, dc;
    u64 ra = 0, rb = 0;
    for (int i = 0; i < 6; i++) sums[i] = 0;
    auto add = [&](u64 &s, u64 v) { s = (s + v) % L.p.q; };
    for (const auto &l : lanes) {      // block_seal_store and block_sum_mod: integer sums, any order
        da.merge(l.ta.seal.s0, l.ta.seal.s1);
        db.merge(l.tb.seal.s0, l.tb.seal.s1);
        dc.merge(l.tc.seal_out.s0, l.tc.seal_out.s1);
        ra += l.ta.n_range;
        rb += l.tb.n_range;
        add(sums[0], A::canonical(l.ta.acc_in, ctx));
        add(sums[1], A::canonical(l.tb.acc_in, ctx));
        add(sums[2], A::canonical(l.ps.acc_a, ctx));
        add(sums[3], A::canonical(l.ps.acc_b, ctx));
        add(sums[4], A::canonical(l.ps.acc_ab, ctx));
        add(sums[5], A::canonical(l.tc.acc_out, ctx));
    }
    const u64 p[8] = {da.s0, da.s1, ra, db.s0, db.s1, rb, dc.s0, dc.s1};
    for (int i = 0; i < 8; i++) parts[i] = p[i];
}

template <class A>
int dispatch_mid(int logn, u64 *a, u64 *b, u64 *c, const Limb &L, int hit_op, long long hit_coeff, int hit_bit, u64 *parts, u64 *sums)
{
    switch (logn) {
#define CASE(LG)                                                                                        \
    case LG:                                                                                            \
        if (hit_op >= 0) emu_mid<A, LG, true>(a, b, c, L, hit_op, hit_coeff, hit_bit, parts, sums);     \
        else emu_mid<A, LG, false>(a, b, c, L, -1, 0, 0, parts, sums);                                  \
        return 0;
        CASE(5) CASE(10)
#undef CASE
    default: return -1;
    }
}

} // namespace

// c = a * b mod (x^N + 1, q) for one limb-polynomial through the sealed single launch.  parts = lazily reduced {S0, S1, n_range} of
// a, the same of b, {S0, S1} of c; sums = the detector's {ain, bin, aout, bout, cin, cout}.  hit_op 0 / 1: the hooked tap flips
// hit_bit of word hit_coeff of a / b as it is loaded (< 0: off).  rp = forward table (entry k = psi^bitrev(k)), w_hat = the ABFT
// weights of the transformed side as residues.  Returns 0, or -1 for a size the emulation is not instantiated for.
extern "C" int emu_polymul_sealed(u64 *a, u64 *b, u64 *c, int logn, u64 q, const u64 *rp, const u64 *w_hat, int path, int hit_op, long long hit_coeff, int hit_bit,
                                  u64 *parts, u64 *sums)
{
    const Limb L(logn, q, rp, w_hat, path);
    return path == PATH_F64 ? dispatch_mid<ArithF64>(logn, a, b, c, L, hit_op, hit_coeff, hit_bit, parts, sums)
                            : dispatch_mid<ArithU64>(logn, a, b, c, L, hit_op, hit_coeff, hit_bit, parts, sums);
}
