// emu_abft.cpp -- CPU emulation of the ABFT taps on the real pass templates (TEST INFRASTRUCTURE ONLY).
//
// Compiles fhe_reliability_gpu_amd/csrc/abft_taps.hpp together with ntt_core.hpp / ntt_plan.hpp with g++ and runs the
// checked inverse transform's passes (InvChecksumTap) and the checked product's per-point sums (ProductSums, on the lazy
// words the product's forward row pass leaves) thread by thread, so that the checksum identities can be checked against
// the oracle without a GPU.  The library never links this file.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I<csrc> emu_abft.cpp -o libemu_abft.so
#include "abft_taps.hpp"
#include "ntt_plan.hpp"

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
    std::vector<Tw> fwd, inv;
    std::vector<Tw> win, wout;      // weights in twiddle encoding (ArithU64 limbs)
    std::vector<u64> wout8;         // output-side weights as residues (ArithF64 limbs)
    Limb(int logn, u64 q, const u64 *rp, const u64 *w_hat, int path)
    {
        const size_t N = (size_t)1 << logn;
        fwd.resize(N);
        inv.resize(N);
        for (size_t k = 0; k < N; k++) {
            const u64 w = rp[k], wi = invmod(w, q);
            const u32 at = tw_stored_index(logn, (u32)k);
            fwd[at] = path == PATH_F64 ? ArithF64::encode(w, q) : ArithU64::encode(w, q);
            inv[at] = path == PATH_F64 ? ArithF64::encode(wi, q) : ArithU64::encode(wi, q);
        }
        const u64 ni = invmod(N % q, q);
        {
            const u64 w1 = invmod(rp[N > 1 ? 1 : 0], q), wn = (u64)((unsigned __int128)ni * w1 % q);
            inv[0] = path == PATH_F64 ? ArithF64::encode(wn, q) : ArithU64::encode(wn, q);
        }
        const u64 p2 = (u64)1 << (logn / 2);
        win.resize(N);
        wout.resize(N);
        wout8.assign(w_hat, w_hat + N);
        for (size_t i = 0; i < N; i++) {
            const u64 wi = ((i % p2 + 1) + (i / p2 + 1)) % q;
            win[i] = path == PATH_F64 ? ArithF64::encode(wi, q) : ArithU64::encode(wi, q);
            wout[i] = path == PATH_F64 ? ArithF64::encode(w_hat[i], q) : ArithU64::encode(w_hat[i], q);
        }
        p.q = q;
        p.two_q = 2 * q;
        p.n = (double)q;
        p.ninv = 1.0 / p.n;
        const unsigned __int128 ratio = ~(unsigned __int128)0 / q;     // floor(2^128 / q), q odd
        p.barrett_lo = (u64)ratio;
        p.barrett_hi = (u64)(ratio >> 64);
        p.inv_n = path == PATH_F64 ? ArithF64::encode(ni, q) : ArithU64::encode(ni, q);
        p.fwd = fwd.data();
        p.inv = inv.data();
        p.path = path;
    }
};

// one pass over every tile of one limb-polynomial, thread by thread, with an optional tap per tile; `sum` collects the
// tiles' canonical sums as the comparison kernel does
template <class PASS, int LOGN, bool INV, bool IS_COL, class TAP>
void emu_pass(u64 *data, const Limb &L, bool tapped, u64 *sum_in, u64 *sum_out)
{
    typedef typename PASS::Arith A;
    PassArgs a{data, &L.p, 0u, 1u, 1u, 1u};
    std::vector<typename PASS::elem> lds(PASS::LDS_ELEMS > 0 ? PASS::LDS_ELEMS : 1);
    for (u32 b = 0; b < PASS::TILES; b++) {
        u32 limb, row0 = 0;
        u64 *base;
        if constexpr (IS_COL) base = col_tile<PASS, LOGN>(b, a, limb);
        else base = row_tile<PASS, LOGN>(b, a, limb, row0);
        const auto ctx = A::make_ctx(L.p);
        const TwPtr tw = as_global(INV ? L.p.inv : L.p.fwd);
        const u32 pos0 = (u32)(base - data);
        TAP tap{L.win.data() + pos0, L.wout.data() + pos0, L.wout8.data() + pos0, pos0, LOGN / 2,
                typename A::elem(0), typename A::elem(0), 0, 0};
        TAP *t = tapped ? &tap : nullptr;
        auto run = [&](auto e) {
            constexpr int E = decltype(e)::value;
            if constexpr (E < PASS::NPHASE) {
                for (int tid = 0; tid < PASS::THREADS; tid++) {
                    if (t) PASS::template phase<E>(tid, base, lds.data(), tw, row0, ctx, L.p.inv_n, t);
                    else PASS::template phase<E>(tid, base, lds.data(), tw, row0, ctx, L.p.inv_n);
                }
            }
        };
        run(std::integral_constant<int, 0>());
        run(std::integral_constant<int, 1>());
        run(std::integral_constant<int, 2>());
        run(std::integral_constant<int, 3>());
        run(std::integral_constant<int, 4>());
        if (tapped) {
            *sum_in = (*sum_in + A::canonical(tap.acc_in, ctx)) % L.p.q;
            *sum_out = (*sum_out + A::canonical(tap.acc_out, ctx)) % L.p.q;
        }
    }
}

// checked inverse: first launch with the input tap, optional bit flip between the launches, last launch with the output tap
template <class A, int LOGN>
void emu_inverse(u64 *data, const Limb &L, long long flip_idx, int flip_bit, u64 *s_in, u64 *s_out)
{
    typedef Passes<A, LOGN, true, (LOGN >= 13 ? 1 : 0)> PS;
    u64 unused = 0;
    if constexpr (!PS::G::TWO_PASS) {
        emu_pass<typename PS::Single, LOGN, true, false, InvChecksumTap<A, true, true>>(data, L, true, s_in, s_out);
    } else {
        emu_pass<typename PS::Row, LOGN, true, false, InvChecksumTap<A, true, false>>(data, L, true, s_in, &unused);
        if (flip_idx >= 0) data[flip_idx] ^= (u64)1 << flip_bit;
        emu_pass<typename PS::Col, LOGN, true, true, InvChecksumTap<A, false, true>>(data, L, true, &unused, s_out);
    }
}

// forward transform of one factor as the checked product runs it: column pass (two-launch sizes, input tap) and the middle
// launch's forward row pass (one-launch sizes: input tap here); the result stays in the row pass's lazy form
template <class A, int LOGN>
void emu_product_forward(u64 *data, const Limb &L, u64 *s_in)
{
    typedef MidPasses<A, LOGN, (LOGN >= 13 ? 1 : 0)> MP;
    u64 unused = 0;
    if constexpr (MP::TWO) {
        emu_pass<typename MP::F::Col, LOGN, false, true, ChecksumTap<A, true, false>>(data, L, true, s_in, &unused);
        emu_pass<typename MP::Fwd, LOGN, false, false, ChecksumTap<A, true, false>>(data, L, false, nullptr, nullptr);
    } else {
        emu_pass<typename MP::Fwd, LOGN, false, false, ChecksumTap<A, true, false>>(data, L, true, s_in, &unused);
    }
}

template <class A, int LOGN>
void emu_product(u64 *a, u64 *b, const Limb &L, u64 *out)
{
    const size_t N = (size_t)1 << LOGN;
    emu_product_forward<A, LOGN>(a, L, &out[0]);
    emu_product_forward<A, LOGN>(b, L, &out[1]);
    const auto ctx = A::make_ctx(L.p);
    ProductSums<A> ps{typename A::elem(0), typename A::elem(0), typename A::elem(0), 0};
    for (size_t j = 0; j < N; j++) {
        const typename A::elem x = A::load_lazy(a[j]), y = A::load_lazy(b[j]);
        if constexpr (A::PATH == PATH_F64) ps.add(x, y, A::from_canonical(L.wout8[j]), ctx);
        else ps.add(x, y, L.wout[j], ctx, L.p);
        // the product as the middle launch forms it, canonical, for the caller's inverse
        typename A::elem c;
        if constexpr (A::PATH == PATH_F64) c = A::mulvar_lazy(x, y, ctx);
        else c = A::mulvar_lazy(x, y, L.p);
        a[j] = A::canonical(c, ctx);
    }
    out[2] = A::canonical(ps.acc_a, ctx);
    out[3] = A::canonical(ps.acc_b, ctx);
    out[4] = A::canonical(ps.acc_ab, ctx);
}

template <class A>
int dispatch(int logn, u64 *x, u64 *y, const Limb &L, long long flip_idx, int flip_bit, u64 *out, bool product)
{
    switch (logn) {
#define CASE(LG)                                                                          \
    case LG:                                                                              \
        if (product) emu_product<A, LG>(x, y, L, out);                                    \
        else emu_inverse<A, LG>(x, L, flip_idx, flip_bit, &out[0], &out[1]);              \
        return 0;
        CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16)
#undef CASE
    default: return -1;
    }
}

} // namespace

// Checked inverse of one limb-polynomial in place: out[0] = sum w^ X over the first launch's loads, out[1] = sum w x over the
// last launch's stores.  rp = forward table (entry k = psi^bitrev(k)), w_hat = output-side weights as residues.  flip_idx >= 0:
// XOR bit flip_bit of that word between the two launches (two-launch sizes).
extern "C" int emu_inverse_checked(u64 *data, int logn, u64 q, const u64 *rp, const u64 *w_hat, int path, long long flip_idx, int flip_bit, u64 *out)
{
    const Limb L(logn, q, rp, w_hat, path);
    out[0] = out[1] = 0;
    return path == PATH_F64 ? dispatch<ArithF64>(logn, data, nullptr, L, flip_idx, flip_bit, out, false)
                            : dispatch<ArithU64>(logn, data, nullptr, L, flip_idx, flip_bit, out, false);
}

// Sums of the checked product for one limb-polynomial: out = {sum w a, sum w b, sum w^ a^, sum w^ b^, sum w^ a^ b^}; a and b are
// transformed in place, and a receives the canonical products a^ b^ (NTT domain).
extern "C" int emu_product_sums(u64 *a, u64 *b, int logn, u64 q, const u64 *rp, const u64 *w_hat, int path, u64 *out)
{
    const Limb L(logn, q, rp, w_hat, path);
    for (int i = 0; i < 5; i++) out[i] = 0;
    return path == PATH_F64 ? dispatch<ArithF64>(logn, a, b, L, -1, 0, out, true) : dispatch<ArithU64>(logn, a, b, L, -1, 0, out, true);
}
