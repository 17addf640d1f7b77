// galois_seal.hpp -- the NTT-domain Galois permutation that verifies its source's seal and writes its destination's on the one load
// a permutation makes (host + device: the kernels of galois_sealed.hip and the CPU emulation tests/emu/emu_galois_seal.cpp compile
// the same functions).
//
// dst[j] = src[pi_k(j)], pi_k = galois_slot(., logn, k) of ntt_core.hpp.  The checked permutation (galois_check.hpp) compares two
// residue sums modulo 2^32 - 1 -- blind to +2^b - 2^(b+32) inside a word -- from two reads of the source, and says nothing about a
// word that was already wrong in memory.  A permutation gathers each source word exactly once, so the register v that is stored at
// slot j is the register that is digested, twice, with the sums of seal_check.hpp modulo p = 2^61 - 1:
//     s0     += v                     S0 of the source AND of the destination: a permutation leaves the plain sum alone
//     s1_in  += (from + 1) v          from = pi_k(j): the word's weight in the SOURCE row, held against the source's seal
//     s1_out += (j + 1) v             its weight in the DESTINATION row, for the destination's seal (kept only when one is asked for)
// and a count of the words >= q_l for the window.  pi_k is a bijection of the row, so over a whole row (s0, s1_in) is the seal of the
// source as loaded and (s0, s1_out) the seal of the destination as stored -- but the source words of one destination chunk lie
// anywhere in the row, so a row's source sums exist only after its chunks' partials are merged.  Integer arithmetic modulo p only,
// lazily reduced (at most p + 7) and made canonical once per row: no sum depends on the grid, the chunking or the merge order.
//
// What the row's verdict (galois_seal_finish) catches, with the seal's own certainty (seal_check.hpp): a change confined to one or
// two words of the source row, at rest or on this call's load (S0 moves, or the window sees it); a wrong source index, which
// fetches x' = src[from'] and weighs it by from' + 1: the row's sums then count x' twice and the word x it should have fetched not
// at all, so S0 moves by x' - x, non-zero on a row of pairwise distinct words.  (Where x' = x the stored row is right as well.)
//
// The seal written for the destination is {the STORED S0 of the source, the digested s1_out}: S0 is carried, not re-digested (the
// rule of seal_carry.hpp).  A row whose S0 moved on this call's load therefore keeps failing every later verification of the
// destination: its words and its seal differ by the same amount ever after.  The remaining hole: a source change that leaves S0
// intact and moves S1 alone (three or more words, or x + p through the window) raises the SOURCE's flag on this call but does not
// poison the destination's seal -- s1_out is digested from the words as loaded, so the destination verifies against them.  The
// caller reads the flags of the call that raised them.
//
// Injection points of the one-shot test hook (fhe_ctx_inject_fault_galois_sealed), one (row, destination word): GAL_AT_WORD = one bit
// of the gathered word in the register, before both digests and the store; GAL_AT_INDEX = one bit (< log N, so the index stays in the
// row) of the source index, before the load and before the source weight is formed.  Memory stays clean.
#pragma once
#include "galois_check.hpp"
#include "seal_check.hpp"

namespace fhe {

// what one lane (one chunk, one row) has accumulated; s1_out only with a destination seal
template <bool OUT> struct GalSealAcc {
    static constexpr int WORDS = OUT ? 4 : 3;      // {s0, s1_in, [s1_out], over}: a job's partials
    u64 s0 = 0, s1_in = 0, s1_out = 0, over = 0;

    // the word v gathered from source slot `from` for destination slot j of a row of limb modulus q
    FHE_HD void add(u64 v, u32 from, u32 j, u64 q)
    {
        const u64 f = seal_fold(v);
        s0 = seal_fold(s0 + f);
        s1_in = seal_fold(s1_in + seal_wmul(f, from + 1));
        if (OUT) s1_out = seal_fold(s1_out + seal_wmul(f, j + 1));
        over += v >= q ? 1 : 0;      // at most N <= 2^30 per row
    }
    // the sums as they travel (shuffles, LDS, the partials in memory): WORDS of them, in the order of a job's partials
    FHE_HD u64 get(int i) const { return i == 0 ? s0 : i == 1 ? s1_in : (OUT && i == 2) ? s1_out : over; }
    FHE_HD void merge(const u64 *o)
    {
        s0 = seal_fold(s0 + seal_fold(o[0]));
        s1_in = seal_fold(s1_in + seal_fold(o[1]));
        if (OUT) s1_out = seal_fold(s1_out + seal_fold(o[2]));
        over += o[WORDS - 1];
    }
};

// destination slot j of one row: gathers, digests and returns the word to store.  word_mask / index_mask: the test hook (0 on every
// element but the armed one)
template <bool OUT> FHE_HD u64 galois_seal_step(GalSealAcc<OUT> &acc, const u64 *src_row, u32 j, int logn, u32 k, u64 q, u64 word_mask, u32 index_mask)
{
    const u32 from = galois_slot(j, logn, k) ^ index_mask;
    const u64 v = src_row[from] ^ word_mask;
    acc.add(v, from, j, q);
    return v;
}

// what the finish step decides for one row: acc = the row's merged sums, stored = the source's seal as it lies in memory (held word
// for word, as fhe_seal_verify holds it: a stored sum that is not canonical counts as moved).  Returns the row's flag bits; with OUT
// seal_dst receives {stored S0, canonical s1_out} -- seal_dst may be `stored` itself
template <bool OUT> FHE_HD u32 galois_seal_finish(const GalSealAcc<OUT> &acc, const u64 *stored, u64 *seal_dst)
{
    const u64 st0 = stored[0], st1 = stored[1];
    u32 flag = 0;
    if (seal_canonical(acc.s0) != st0 || seal_canonical(acc.s1_in) != st1) flag |= SEAL_SUM;
    if (acc.over) flag |= SEAL_RANGE;
    if (OUT) {
        seal_dst[0] = st0;
        seal_dst[1] = seal_canonical(acc.s1_out);
    }
    return flag;
}

} // namespace fhe
