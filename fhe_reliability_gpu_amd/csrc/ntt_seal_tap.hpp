// ntt_seal_tap.hpp -- the seal of a transform's input, digested from the words the transform's first launch reads, and the seal of
// its output, digested from the words its last launch stores (host + device: k_ntt_pass_sealed_io of ntt_sealed_io.hpp and the CPU
// emulation tests/emu/emu_ntt_seal.cpp compile the same tap with the same pass templates).
//
// The sealed streaming kernels digest an operand from the register that is then consumed.  The input limbs of a key switch are
// consumed by a transform: its first launch (the inverse row pass, or the single pass below 2^13) reads them.  SealTap is the
// checked transform's tap (abft_taps.hpp InvChecksumTap / ChecksumTap) plus the seal of seal_check.hpp over the same
// words: the pass hands every raw 64-bit word of its first register step to raw() BEFORE the conversion to the arithmetic's
// element (ntt_core.hpp tap_sees_raw) -- on the FP64 path a corrupted word above 2^53 does not survive that conversion, so the
// digest cannot be taken from the element.  The word's weight is its index in the row plus one, as in every seal; words >= q_l
// are counted (the window).  in() and the ABFT sum are the base's, unchanged: they see the converted element.
//
// What is covered: the word as the first register step holds it -- after the load from memory and, where the pass stages its
// tile through LDS (rows of 32 points and more), after that staging.  Not covered: a fault between raw()'s read of the register
// and the conversion that consumes the same register.
//
// HOOK: the one-shot test fault of fhe_ctx_inject_fault_ntt_sealed, a one-word XOR at (row, index) applied inside raw() before
// window, digest and conversion; memory stays clean.
//
// The sealed forward transform and the inverse with an output seal (fhe_ntt_forward_sealed, fhe_ntt_inverse_sealed_out) are the
// same tap over either ABFT base.  Input side: raw() as above, on the forward column pass
// (N >= 2^13) or the single pass -- ColPass hands its first register step's words to raw() exactly as RowPass does.  A word >= q_l
// is digested as it is and raises SEAL_RANGE; the transform then reduces it as the unchecked transform does.  Output side: out()
// is called with every final word on its way to memory (RowPass::copy_out, the TO_GLOBAL branch of the single pass, ColPass's last
// step); besides the base's ABFT sum it digests that word with weight pos0 + idx + 1, its index in the STORED row (the engine's
// bit-reversed order for the forward transform), so the merged digest is fhe_seal's of the output row, word for word.
//
// The poison rule (ntt_seal_out): a row whose input verdict or ABFT flag is raised leaves the call with the seal {~0, ~0}.  Neither
// word is canonical, and every verifier holds a stored sum word for word against a canonical one (seal_differs, seal_decide), so
// A ROW WITH ANY RAISED FLAG LEAVES THE CALL WITH A SEAL THAT CAN NEVER VERIFY: the row stays raised in every later verification,
// and repair reports it SEAL_UNCORRECTABLE.
#pragma once
#include "abft_taps.hpp"
#include "seal_check.hpp"

#include <type_traits>

namespace fhe {

constexpr u32 NTT_SEAL_NO_HIT = 0xFFFFFFFFu;
// words of one (row, tile) partial: S0, S1 (lazily reduced), the count of words >= q_l
constexpr int NTT_SEAL_PART = 3;

// BASE = the ABFT tap of the pass (abft_taps.hpp); IN: raw() digests the words a first register step takes; OUT: out() digests the
// final words on their way to memory, after BASE's own out()
template <class BASE, bool HOOK, bool IN, bool OUT>
struct SealTap : BASE {
    static constexpr bool SEES_RAW = IN;
    SealAcc seal;
    u32 n_range;
    u64 q;
    u32 hit_idx;      // HOOK: index of the word to flip, relative to the tile's first word (NTT_SEAL_NO_HIT: none in this tile)
    u64 hit_mask;
    SealAcc seal_out;
    FHE_D void raw(u32 idx, u64 &w)
    {
        if constexpr (IN) {
            if constexpr (HOOK) {
                if (idx == hit_idx) w ^= hit_mask;
            }
            n_range += w >= q ? 1u : 0u;
            seal.add(w, this->pos0 + idx);
        }
    }
    template <class CTX> FHE_D void out(u32 idx, u64 v, const CTX &c)
    {
        BASE::out(idx, v, c);
        if constexpr (OUT) seal_out.add(v, this->pos0 + idx);
    }
};

// the hooked word's index relative to the first word of the tile at pos0, as raw() is handed it, or NTT_SEAL_NO_HIT where the tile
// does not hold word hit_coeff of its row: a column tile holds TCOLS adjacent words out of every STRIDE, a row tile TROWS * NPTS
// adjacent words
template <class PASS, bool IS_COL> FHE_HD u32 ntt_seal_tile_hit(u32 hit_coeff, u32 pos0)
{
    const u32 d = hit_coeff - pos0;
    if constexpr (IS_COL) return (d & (PASS::STRIDE - 1u)) < (u32)PASS::TCOLS ? d : NTT_SEAL_NO_HIT;
    else return d < (u32)(PASS::TROWS * PASS::NPTS) ? d : NTT_SEAL_NO_HIT;
}

// the tap of a sealed pass (k_ntt_pass_sealed_io): the ABFT sums of the direction's base on the sides IN / OUT, the input digest
// where IN, the output digest where DIGEST -- OUT without DIGEST is the inverse single pass of a call that writes no output seal
template <class A, bool INV, bool HOOK, bool IN, bool OUT, bool DIGEST = OUT>
using SealPassTap = SealTap<std::conditional_t<INV, InvChecksumTap<A, IN, OUT>, ChecksumTap<A, IN, OUT>>, HOOK, IN, DIGEST>;
// the names the tap's three uses had before there was one kernel, kept for code written against them: the sealed inverse's first
// launch without an output digest, the forward transform, the inverse with an output seal
template <class A, bool HOOK, bool OUT = false> using SealInTap = SealPassTap<A, true, HOOK, true, OUT, false>;
template <class A, bool HOOK, bool IN, bool OUT> using SealFwdTap = SealPassTap<A, false, HOOK, IN, OUT>;
template <class A, bool HOOK, bool IN, bool OUT> using SealInvTap = SealPassTap<A, true, HOOK, IN, OUT>;

// a row's merged partials against its stored seal: SEAL_SUM where a canonical sum differs word for word from the stored one (a
// stored sum that is not canonical therefore counts as different; stored == nullptr: not compared), SEAL_RANGE where a word was
// >= q_l
FHE_HD u32 ntt_seal_verdict(const SealAcc &acc, u64 n_range, const u64 *stored)
{
    u32 f = n_range ? (u32)SEAL_RANGE : 0u;
    if (stored && (seal_canonical(acc.s0) != stored[0] || seal_canonical(acc.s1) != stored[1])) f |= (u32)SEAL_SUM;
    return f;
}

// words of one (row, tile) partial of the output digest: S0, S1 (lazily reduced)
constexpr int NTT_SEAL_OUT_PART = 2;
constexpr u64 NTT_SEAL_POISON = ~(u64)0;

// the seal a row leaves the call with: its merged output digest, canonical, where the row's input verdict and its ABFT flag are
// both zero; otherwise the poisoned pair, which no verifier accepts
FHE_HD void ntt_seal_out(const SealAcc &acc, u32 flag_in, u32 flag_abft, u64 *seal)
{
    const bool ok = flag_in == 0 && flag_abft == 0;
    seal[0] = ok ? seal_canonical(acc.s0) : NTT_SEAL_POISON;
    seal[1] = ok ? seal_canonical(acc.s1) : NTT_SEAL_POISON;
}

} // namespace fhe
