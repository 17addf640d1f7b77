// ntt_inv_sealed_out.hip -- the sealed inverse transform with its output's seal written from the words it stores
// (ntt_seal_tap.hpp, ntt_sealed_io.hpp): fhe_ntt_inverse_sealed_out.  A translation unit of its own, so that every other kernel,
// fhe_ntt_inverse_sealed's included, compiles exactly as before.
//
// Two-launch sizes (N >= 2^13): the first launch is k_ntt_pass_sealed with its verdict (launch_ntt_sealed_inv, which = 0), the
// last launch is the inverse column pass with the output digest over InvChecksumTap.  Below 2^13 the inverse single pass carries
// the input digest and the output digest in one launch.  The rows' seals are written by k_ntt_seal_out_finish (ntt_fwd_sealed.hip)
// after launch_compare_sums, by the same poison rule.
#include "ntt_sealed_io.hpp"

namespace fhe {

namespace {

template <class A, int LOGN>
hipError_t launch_sealed_inv_out_t(hipStream_t st, const PassArgs &a, const SealIoArgs &sp, int path, int which, const NttSealIn &s)
{
    constexpr int GEO = LOGN >= 13 ? 1 : 0;
    typedef Passes<A, LOGN, true, GEO> PS;
    if constexpr (!PS::G::TWO_PASS) {
        if (which == 1) return hipSuccess;
        hipError_t e = launch_sealed_io<typename PS::Single, LOGN, false, true, true, true>(st, a, sp);
        return e != hipSuccess ? e : launch_ntt_seal_finish(st, a, (u32)PS::Single::TILES, s);
    } else {
        if (which != 1) {
            hipError_t e = launch_ntt_sealed_inv(st, a, sp.win, sp.wout, sp.wout8, sp.sum_in, sp.sum_out, LOGN, path, 0, s);
            if (e != hipSuccess) return e;
        }
        if (which != 0) {
            PassArgs second = a;      // the column pass works in place on what the row pass left in a.data
            second.src = nullptr;
            return launch_sealed_io<typename PS::Col, LOGN, true, true, false, true>(st, second, sp);
        }
        return hipSuccess;
    }
}

} // namespace

hipError_t launch_ntt_sealed_inv_out(hipStream_t st, const PassArgs &a, const Tw *win, const Tw *wout, const u64 *wout8, u64 *sum_in, u64 *sum_out, int logn,
                                     int path, int which, const NttSealIn &s, u64 *part_out)
{
    if (!part_out) return launch_ntt_sealed_inv(st, a, win, wout, wout8, sum_in, sum_out, logn, path, which, s);
    if (a.units == 0) return hipSuccess;
    if (a.map || a.scratch || a.tmp || a.src_bcast || a.src_stride || a.stream_hint || a.galois || a.galois_copy || !s.part || !s.flags) return hipErrorInvalidValue;
    const SealIoArgs sp{win, wout, wout8, logn / 2, sum_in, sum_out, s.part, part_out, s.hit_row, s.hit_coeff, s.hit_mask};
    switch (logn) {
#define FHE_CASE(L) \
    case L: return path == PATH_F64 ? launch_sealed_inv_out_t<ArithF64, L>(st, a, sp, path, which, s) : launch_sealed_inv_out_t<ArithU64, L>(st, a, sp, path, which, s);
        FHE_CASE(5) FHE_CASE(6) FHE_CASE(7) FHE_CASE(8) FHE_CASE(9) FHE_CASE(10) FHE_CASE(11) FHE_CASE(12) FHE_CASE(13)
        FHE_CASE(14) FHE_CASE(15) FHE_CASE(16) FHE_CASE(17) FHE_CASE(18) FHE_CASE(19) FHE_CASE(20)
#undef FHE_CASE
    default: return hipErrorInvalidValue;
    }
}

} // namespace fhe
