// emu_ntt_fwd_seal.cpp -- CPU emulation of the sealed forward transform and of the sealed inverse with an output seal (TEST
// INFRASTRUCTURE ONLY).
//
// Runs every launch of the transform tile by tile, thread by thread, with SealPassTap (ntt_seal_tap.hpp) on the very pass templates
// k_ntt_pass_sealed_io instantiates: the launch that loads the input out of place from a source array with the input digest (and
// the hook), the launch that stores the result with the output digest; below 2^13 one pass with both.  The limb's tables, the tile
// runner and the launch (emu_launch) are emu_ntt_seal.cpp's, included as they are.  The library never links this file.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I<csrc> emu_ntt_fwd_seal.cpp -o libemu_ntt_fwd_seal.so
#include "emu_ntt_seal.cpp"

namespace {

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
        CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16) CASE(17) CASE(18) CASE(19) CASE(20)
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
