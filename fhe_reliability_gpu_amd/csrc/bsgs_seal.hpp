// bsgs_seal.hpp -- the BSGS inner sum's names for the sealed two-half inner product of mac_seal.hpp, where all of it lives: the
// launch's hit record, and the form the CPU emulation tests/emu/emu_bsgs_seal.cpp calls the pair step in (row b of a lane's record =
// the diagonal of baby step b).
#pragma once
#include "bsgs_check.hpp"
#include "mac_seal.hpp"

namespace fhe {

// the one-shot test fault of fhe_ctx_inject_fault_bsgs_sealed as launch_diag_mac_sealed takes it: XOR mask into word coeff of row
// `limb` of diagonal b, in the register as loaded (mask == 0: not armed)
struct DiagHit {
    u32 b, limb;
    u64 coeff, mask;
};

template <class D, int NB, bool HOOK, class LD>
FHE_HD void diag_seal_pair(SealRows<NB> &g, u32 n1, u32 j, const LimbParams &p, const LD &ld, const DiagHit &hit, const PwFault *f0, const PwFault *f1, u64 *c0,
                           u64 *c1, u32 &fl0, u32 &fl1)
{
    mac_seal_pair<D, DiagSealFamily, NB, HOOK>(g, n1, j, p, ld, MacSealHit{hit.b, hit.coeff, hit.mask}, f0, f1, c0, c1, fl0, fl1);
}

template <int NB> using DiagSeal = SealRows<NB>;
FHE_HD bool diag_seal_decide(u64 s0, u64 s1, const u64 *stored) { return seal_differs(s0, s1, stored); }

} // namespace fhe
