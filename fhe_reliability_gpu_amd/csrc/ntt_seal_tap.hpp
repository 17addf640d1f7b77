// ntt_seal_tap.hpp -- the seal of a transform's input, digested from the words the inverse transform's first launch reads (host +
// device: the kernels of ntt_sealed.hip and the CPU emulation tests/emu/emu_ntt_seal.cpp compile the same tap with the same pass
// templates).
//
// The sealed streaming kernels digest an operand from the register that is then consumed.  The input limbs of a key switch are
// consumed by a transform: its first launch (the inverse row pass, or the single pass below 2^13) reads them.  SealInTap is the
// checked inverse's input-side tap (abft_taps.hpp InvChecksumTap<A, true, OUT>) plus the seal of seal_check.hpp over the same
// words: the pass hands every raw 64-bit word of its first register step to raw() BEFORE the conversion to the arithmetic's
// element (ntt_core.hpp tap_sees_raw) -- on the FP64 path a corrupted word above 2^53 does not survive that conversion, so the
// digest cannot be taken from the element.  The word's weight is its index in the row plus one, as in every seal; words >= q_l
// are counted (the window).  in() and the ABFT sum are InvChecksumTap's, unchanged: they see the converted element.
//
// What is covered: the word as the first register step holds it -- after the load from memory and, where the pass stages its
// tile through LDS (rows of 32 points and more), after that staging.  Not covered: a fault between raw()'s read of the register
// and the conversion that consumes the same register.
//
// HOOK: the one-shot test fault of fhe_ctx_inject_fault_ntt_sealed, a one-word XOR at (row, index) applied inside raw() before
// window, digest and conversion; memory stays clean.
#pragma once
#include "abft_taps.hpp"
#include "seal_check.hpp"

namespace fhe {

constexpr u32 NTT_SEAL_NO_HIT = 0xFFFFFFFFu;
// words of one (row, tile) partial: S0, S1 (lazily reduced), the count of words >= q_l
constexpr int NTT_SEAL_PART = 3;

template <class A, bool HOOK, bool OUT = false>
struct SealInTap : InvChecksumTap<A, true, OUT> {
    static constexpr bool SEES_RAW = true;
    SealAcc seal;
    u32 n_range;
    u64 q;
    u32 hit_idx;      // HOOK: index of the word to flip, relative to the tile's first word (NTT_SEAL_NO_HIT: none in this tile)
    u64 hit_mask;
    FHE_D void raw(u32 idx, u64 &w)
    {
        if constexpr (HOOK) {
            if (idx == hit_idx) w ^= hit_mask;
        }
        n_range += w >= q ? 1u : 0u;
        seal.add(w, this->pos0 + idx);
    }
};

// a row's merged partials against its stored seal: SEAL_SUM where a canonical sum differs word for word from the stored one (a
// stored sum that is not canonical therefore counts as different; stored == nullptr: not compared), SEAL_RANGE where a word was
// >= q_l
FHE_HD u32 ntt_seal_verdict(const SealAcc &acc, u64 n_range, const u64 *stored)
{
    u32 f = n_range ? (u32)SEAL_RANGE : 0u;
    if (stored && (seal_canonical(acc.s0) != stored[0] || seal_canonical(acc.s1) != stored[1])) f |= (u32)SEAL_SUM;
    return f;
}

} // namespace fhe
