// emu_gs_abft.cpp -- CPU emulation of the checked natural-order (four-step) transform's taps on the real pass templates
// (TEST INFRASTRUCTURE ONLY).
//
// Compiles fhe_reliability_gpu_amd/csrc/abft_taps.hpp (GsTap) together with ntt_core.hpp / ntt_plan.hpp with g++ and runs the two
// launches of the natural-order transform -- the gathering inverse row pass and the inverse column pass, GsPasses -- thread by
// thread with the taps attached, so that the index mapping of the gathering launch, the hand-off layout and the three checksum
// identities can be checked against Python integers without a GPU.  The library never links this file.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I<csrc> emu_gs_abft.cpp <csrc>/host_math.cpp -o libemu_gs_abft.so
#include "abft_taps.hpp"
#include "host_math.hpp"
#include "ntt_plan.hpp"

#include <vector>

using namespace fhe;

namespace {

Tw enc(int path, u64 w, u64 q) { return path == PATH_F64 ? ArithF64::encode(w, q) : ArithU64::encode(w, q); }

// the natural-order table set of one modulus as the library uploads it (capi.cpp build_tables with gs_scale = 1) and the weights
struct Plan1 {
    LimbParams p;
    std::vector<Tw> fwd, inv, u, m, v;
    Plan1(int logn, u64 q, u64 g, const u64 *u8, const u64 *m8, const u64 *v8, int path)
    {
        const size_t N = (size_t)1 << logn;
        std::vector<u64> row(N);
        host::cyclic_table(q, logn, g, false, row.data());
        fwd.resize(N);
        inv.resize(N);
        for (size_t k = 0; k < N; k++) fwd[tw_stored_index(logn, (u32)k)] = enc(path, row[k] % q, q);
        for (size_t k = 1; k < N; k++) inv[tw_stored_index(logn, (u32)k)] = enc(path, row[k] % q, q);
        inv[tw_stored_index(logn, 0)] = enc(path, row[1 % N] % q, q);
        u.resize(N);
        m.resize(N);
        v.resize(N);
        for (size_t i = 0; i < N; i++) {
            u[i] = enc(path, u8[i], q);
            m[i] = enc(path, m8[i], q);
            v[i] = enc(path, v8[i], q);
        }
        p = LimbParams{};
        p.q = q;
        p.two_q = 2 * q;
        p.n = (double)q;
        p.ninv = 1.0 / p.n;
        const unsigned __int128 ratio = ~(unsigned __int128)0 / q;
        p.barrett_lo = (u64)ratio;
        p.barrett_hi = (u64)(ratio >> 64);
        p.inv_n = enc(path, 1 % q, q);
        p.fwd = fwd.data();
        p.inv = inv.data();
        p.path = path;
    }
};

template <class PASS, class TAP, int E = 0>
void run_phases(u64 *base, typename PASS::elem *lds, TwPtr tw, u32 row0, const typename PASS::Arith::Ctx &ctx, const Tw &inv_n, TAP *tap, const u64 *from)
{
    if constexpr (E < PASS::NPHASE) {
        for (int tid = 0; tid < PASS::THREADS; tid++) PASS::template phase<E>(tid, base, lds, tw, row0, ctx, inv_n, tap, from);
        run_phases<PASS, TAP, E + 1>(base, lds, tw, row0, ctx, inv_n, tap, from);
    }
}

template <class A, int LOGN>
void emu_gs(u64 *dst, const u64 *src, const Plan1 &L, const u64 *u8, const u64 *m8, long long flip_idx, int flip_bit, u64 *out, u64 *handoff)
{
    typedef GsPasses<A, LOGN> GP;
    typedef typename GP::First First;
    constexpr int P = First::P, S0 = First::S0;
    const size_t N = (size_t)1 << LOGN;
    const u64 q = L.p.q;
    const auto ctx = A::make_ctx(L.p);
    const TwPtr tw = as_global(L.p.inv);
    std::vector<u64> tmp(N);
    u64 *first_out = GP::TWO ? tmp.data() : dst;
    {
        typedef GsTap<A, 0, P, S0, true, true> Tap;
        std::vector<typename First::elem> lds(First::LDS_ELEMS);
        for (u32 tile = 0; tile < (u32)First::TILES; tile++) {
            const u32 row0 = tile * First::TROWS;
            Tap tap{L.u.data(), L.m.data(), L.v.data(), u8, m8, row0, LOGN / 2, typename A::elem(0), typename A::elem(0), 0, 0};
            run_phases<First, Tap>(first_out, lds.data(), tw, row0, ctx, L.p.inv_n, &tap, src);
            out[0] = (out[0] + A::canonical(tap.acc_a, ctx)) % q;
            if (GP::TWO) out[1] = (out[1] + A::canonical(tap.acc_b, ctx)) % q;
            else out[3] = (out[3] + A::canonical(tap.acc_b, ctx)) % q;
        }
    }
    if constexpr (GP::TWO) {
        typedef typename GP::Second Col;
        typedef GsTap<A, 1, P, S0, true, true> Tap;
        if (handoff)
            for (size_t i = 0; i < N; i++) handoff[i] = tmp[i];
        if (flip_idx >= 0) tmp[flip_idx] ^= (u64)1 << flip_bit;
        std::vector<typename Col::elem> lds(Col::LDS_ELEMS);
        PassArgs a{dst, &L.p, 0u, 1u, 1u, 1u};
        for (u32 b = 0; b < (u32)Col::TILES; b++) {
            u32 limb;
            u64 *base = col_tile<Col, LOGN>(b, a, limb);
            const u32 pos0 = (u32)(base - dst);
            Tap tap{L.u.data(), L.m.data(), L.v.data(), u8, m8, pos0, LOGN / 2, typename A::elem(0), typename A::elem(0), 0, 0};
            run_phases<Col, Tap>(base, lds.data(), tw, 0u, ctx, L.p.inv_n, &tap, tmp.data() + pos0);
            out[2] = (out[2] + A::canonical(tap.acc_a, ctx)) % q;
            out[3] = (out[3] + A::canonical(tap.acc_b, ctx)) % q;
        }
    }
}

template <class A>
int dispatch(int logn, u64 *dst, const u64 *src, const Plan1 &L, const u64 *u8, const u64 *m8, long long flip_idx, int flip_bit, u64 *out, u64 *handoff)
{
    switch (logn) {
#define CASE(LG) \
    case LG: emu_gs<A, LG>(dst, src, L, u8, m8, flip_idx, flip_bit, out, handoff); return 0;
        CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16)
#undef CASE
    default: return -1;
    }
}

} // namespace

// Checked natural-order transform of one vector, dst = W src (dst may equal src): out = {sum u x over launch 1's loads, sum m z over
// the lazy words launch 1 stores, sum m z over the words launch 2 loads, sum v y over the canonical words stored}; single-launch
// sizes fill out[0] and out[3] only.  u, m, v = the weights as residues.  flip_idx >= 0: XOR bit flip_bit of that hand-off word
// between the launches.  handoff (optional, N words): the hand-off buffer as launch 1 left it.
extern "C" int emu_gs_checked(u64 *dst, const u64 *src, int logn, u64 q, u64 g, const u64 *u, const u64 *m, const u64 *v, int path, long long flip_idx,
                              int flip_bit, u64 *out, u64 *handoff)
{
    const Plan1 L(logn, q, g, u, m, v, path);
    for (int i = 0; i < 4; i++) out[i] = 0;
    return path == PATH_F64 ? dispatch<ArithF64>(logn, dst, src, L, u, m, flip_idx, flip_bit, out, handoff)
                            : dispatch<ArithU64>(logn, dst, src, L, u, m, flip_idx, flip_bit, out, handoff);
}
