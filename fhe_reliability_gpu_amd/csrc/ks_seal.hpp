// ks_seal.hpp -- the key switch's names for the sealed two-half inner product of mac_seal.hpp, where all of it lives: the form the
// CPU emulation tests/emu/emu_ks_seal.cpp calls it in (row 2 d + h of a lane's record = half h of digit d).
#pragma once
#include "mac_seal.hpp"

namespace fhe {

// MacSealHit with the slot split into digit and half (d past every digit: not this row)
struct KsHit {
    u32 d, h;
    u64 coeff, mask;
};

template <class D, int ND, bool HOOK, class LD>
FHE_HD void ks_seal_pair(SealRows<2 * ND> &g, u32 dnum, u32 j, const LimbParams &p, const LD &ld, const KsHit &hit, const PwFault *f0, const PwFault *f1, u64 *c0,
                         u64 *c1, u32 &fl0, u32 &fl1)
{
    mac_seal_pair<D, KsSealFamily, ND, HOOK>(g, dnum, j, p, ld, MacSealHit{2 * hit.d + hit.h, hit.coeff, hit.mask}, f0, f1, c0, c1, fl0, fl1);
}

template <int ND> using KsSeal = SealRows<2 * ND>;
FHE_HD bool ks_seal_decide(u64 s0, u64 s1, const u64 *stored) { return seal_differs(s0, s1, stored); }

} // namespace fhe
