// subscale_seal.hpp -- the mod-down tail with its first operand verified on the load that subtracts from it and its result sealed
// from the register that is stored (host + device: the kernels of subscale_sealed.hip and the CPU emulation
// tests/emu/emu_subscale_seal.cpp compile the same functions).
//
// k_sub_scale_checked (keyswitch_checked.hip) ends every checked key switch (stage 7) and every checked rescale (stage 3):
//     out = ((x - y mod q) s mod q + add) mod q
// It loads each word of x once and stores each word of out once.  A caller with a sealed x could only sweep x before the call, and
// a sealed composite could only sweep out after it: the verifying load and the consuming load, the store and the sealing load were
// different ones, and a word that is wrong on the second of each pair passes.  Here the seal of seal_check.hpp (S0 = sum x_j, S1 =
// sum (j + 1) x_j modulo p = 2^61 - 1, and the window x_j < q) is digested
//   IN:  from the register that is then handed to checked_sub_scale as x -- the verified load IS the consuming load;
//   OUT: from the register that checked_sub_scale returned and that is then stored -- the sealed word IS the stored word.
// y (the plan's own residues) and the addends (the caller's own in fhe_keyswitch_apply_*) are not digested.
//
// The arithmetic is checked_sub_scale's, unchanged: the same call per word, the same operands present or absent, the same residue
// flags and PW_AT_* fault points; the words are k_sub_scale's bit for bit -- also for an x word >= q: the call flags such a word
// (the window bit here, PW_OPERAND in the residue flags), it does not fix it.  Integer arithmetic modulo p throughout the digest:
// it does not depend on how a row is cut into chunks, lanes or waves, nor on the order in which partial sums are merged.
#pragma once
#include "keyswitch_check.hpp"
#include "seal_check.hpp"

namespace fhe {

// the points of the one-shot test fault of fhe_ctx_inject_fault_subscale_sealed
//   SS_AT_LOAD   one bit of an x word in the register as loaded: before the window, the digest and the arithmetic read it (IN)
//   SS_AT_STORE  one bit of the result word in the register after its digest and before its store (OUT)
enum { SS_AT_LOAD = 0, SS_AT_STORE = 1 };

// the fault as one word's step reads it: mask == 0 for every word but the target
struct SubScaleHit {
    int point;      // < 0: none
    u64 mask;
};

// the operands of one word as SubScaleArgs' pointers give them: an absent one is zero and has_* false
struct SubScaleWord {
    u64 x, y, add;
    bool has_x, has_y, has_add;
};

// the digests a lane keeps for the row it works on: the row of x as loaded (IN) and the row of out as stored (OUT), in that order
template <bool IN, bool OUT> using SubScaleSealAcc = SealRows<(IN ? 1 : 0) + (OUT ? 1 : 0)>;

// One word, index j of its row: digests x into g.acc[0] and holds it against the window (IN; g.range bit 0), forms the word with
// checked_sub_scale, digests it into the last row of g (OUT) and returns it as it is to be stored.  flags |= the residue flags.
template <bool IN, bool OUT, bool HOOK>
FHE_HD u64 sub_scale_seal_word(SubScaleSealAcc<IN, OUT> &g, SubScaleWord w, u32 j, u64 s, u64 q, u64 r0, u64 r1, u32 rq, u32 &flags, const PwFault &f,
                               const SubScaleHit &hit)
{
    if (HOOK && IN && hit.point == SS_AT_LOAD) w.x ^= hit.mask;
    if (IN) {
        g.acc[0].add(w.x, j);
        g.range |= w.x >= q ? 1u : 0u;
    }
    u32 fl;
    u64 v = checked_sub_scale(w.x, w.has_x, w.y, w.has_y, s, w.add, w.has_add, q, r0, r1, rq, fl, f);
    flags |= fl;
    if (OUT) g.acc[IN ? 1 : 0].add(v, j);
    if (HOOK && OUT && hit.point == SS_AT_STORE) v ^= hit.mask;
    return v;
}

// what the finish step decides for the x row: s0 / s1 = its lazily reduced digests, stored = its seal as it lies in memory (null: not
// compared), range = a word was >= q
FHE_HD u32 sub_scale_seal_verdict(u64 s0, u64 s1, bool range, const u64 *stored)
{
    return (range ? (u32)SEAL_RANGE : 0u) | (stored && seal_differs(s0, s1, stored) ? (u32)SEAL_SUM : 0u);
}

// does a fault at `point` fit a launch: SS_AT_LOAD needs the IN form, SS_AT_STORE the OUT form
FHE_HD bool sub_scale_seal_point_exists(int point, bool in, bool out) { return (point == SS_AT_LOAD && in) || (point == SS_AT_STORE && out); }

} // namespace fhe
