// rescale_round.hpp -- the per-word step of the round-to-nearest rescale, shared by the HIP kernels (ntt_kernels.hip: the column
// pass that takes the last limb's residues on its load, the second input of k_ntt_col_addsrc; aux_kernels.hip: the residues of the
// sizes below 2^13) and the CPU emulation of the tests (tests/emu/emu_rescale_round.cpp).
//
// One coefficient of the last limb in coefficient form is a word y in [0, q), q = q_{L-1} odd, h = (q - 1) / 2.  The nearest rescale
// removes the CENTRED remainder r = y (y <= h) or y - q (y > h), r in [-h, h], where the flooring one removes y itself:
//   floor((C + h) / q) = (C - r) / q.
// What a limb j < L-1 needs is r mod q_j.  |r| <= h, so the magnitude is reduced and the sign put back afterwards: no constant
// per limb (SEAL's h mod q_j) is needed, q and h travel as launch arguments, and where q < 2 q_j -- primes of one size -- the
// magnitude is below q_j already and no division runs at all.  The result is the canonical word in [0, q_j): exact input of both
// arithmetic paths (ArithF64 takes canonical words below 2^50 through from_canonical, ArithU64 as they are).
#pragma once
#include "modarith.hpp"

namespace fhe {

// y < q, h = (q - 1) / 2, any size relation between q and qj (both below 2^61)
FHE_HD u64 round_residue(u64 y, u64 q, u64 h, u64 qj)
{
    const bool neg = y > h;
    const u64 m = neg ? q - y : y;                               // |r| <= h
    const u64 t = __builtin_expect(m < qj, 1) ? m : reduce_any_u64(m, qj);      // cold: only a last prime of twice q_j or more gets here
    return neg && t ? qj - t : t;
}

} // namespace fhe
