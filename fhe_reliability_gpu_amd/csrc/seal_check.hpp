// seal_check.hpp -- the seal of a row at rest: two position-weighted sums modulo the Mersenne prime p = 2^61 - 1 (host + device:
// the kernels of seal_checked.hip and the CPU emulation tests/emu/emu_seal_check.cpp compile the same functions).
//
// The checked calls start from the registers they loaded, so a word that was already wrong in memory -- the bit flips of
// reliability_test/dotprod_test.cu:31-61, a word that rots between one call's store and the next call's load, a flipped word of a
// switching key -- is a perfectly consistent input to every stage.  A seal travels with a ciphertext or key between calls: per row
// of N words x_0 .. x_(N-1) of limb l
//     S0 = sum_j x_j mod p,      S1 = sum_j (j + 1) x_j mod p,      and the window x_j < q_l,
// stored as uint64_t [rows][2], canonical in [0, p) (the value p itself is 0).
//
// Why not the fold modulo m = 2^32 - 1 of residue_check.hpp: m is composite and 2^32 = 1 modulo m, so a multi-bit change such as
// +2^b - 2^(b+32) inside one word is invisible to it, and the reference flips several bits per symbol.  With p prime and every
// canonical word below q < 2^61 <= p:
//   a change confined to ONE word of a row is caught with certainty: either the new word is >= q (the window), or the difference
//     d = x' - x is non-zero with |d| < q <= p, so S0 moves;
//   a change confined to TWO words j1 != j2 is caught with certainty: unseen by the window, d1 + d2 = 0 and
//     (j1 + 1) d1 + (j2 + 1) d2 = 0 modulo p give (j1 - j2) d1 = 0, and 0 < |j1 - j2| < N < p, 0 < |d1| < p with p prime force d1 = 0;
//   wider corruption escapes with probability about 2^-61 per sum on random data.
// A seal says nothing about WHO wrote the row: it is an integrity record against faults, not an authentication code.
//
// Arithmetic: 2^61 = 1 modulo p, so x mod p folds as (x & p) + (x >> 61).  All sums are kept lazily reduced (at most p + 7) and are
// made canonical once, at the end: integer addition modulo p is associative and commutative, so the seal does not depend on how a
// row is cut into chunks, lanes or waves, nor on the order in which partial sums are combined.  The weight of a word is its index
// in the ROW (plus one), whatever chunk it was read in.  One 61 x 32-bit product per word, no floating point.
#pragma once
#include "modarith.hpp"

namespace fhe {

constexpr u64 SEAL_P = ((u64)1 << 61) - 1;
enum { SEAL_SUM = 1, SEAL_RANGE = 2 };      // flag bits of a verification: a sum differs, a word >= q_l
// a row is swept in chunks of at most 2^SEAL_LOG_CHUNK words, one workgroup per chunk at a time
constexpr int SEAL_LOG_CHUNK = 13;

// x mod p, lazily: any 64-bit x -> at most p + 7
FHE_HD u64 seal_fold(u64 x) { return (x & SEAL_P) + (x >> 61); }

// w x mod p, lazily, for a folded x (<= p + 7) and a 32-bit weight: the 94-bit product as two 32 x 32 -> 64-bit multiply-adds,
// its low 61 bits plus the rest; below 2^61 + 2^33
FHE_HD u64 seal_wmul(u64 x, u32 w)
{
    const u64 lo = (x & 0xFFFFFFFFu) * w;
    const u64 hi = (x >> 32) * w + (lo >> 32);      // the product is hi 2^32 + (lo mod 2^32)
    return (((hi << 32) | (lo & 0xFFFFFFFFu)) & SEAL_P) + (hi >> 29);
}

// the two running sums, each at most p + 7 between calls
struct SealAcc {
    u64 s0 = 0, s1 = 0;
    // word x at index j of its row: weight j + 1
    FHE_HD void add(u64 x, u32 j)
    {
        const u64 f = seal_fold(x);
        s0 = seal_fold(s0 + f);
        s1 = seal_fold(s1 + seal_wmul(f, j + 1));
    }
    FHE_HD void merge(u64 o0, u64 o1)
    {
        s0 = seal_fold(s0 + seal_fold(o0));
        s1 = seal_fold(s1 + seal_fold(o1));
    }
};

// a lazily reduced sum -> [0, p): two folds bring any 64-bit value to at most p, and p itself is 0
FHE_HD u64 seal_canonical(u64 s)
{
    s = seal_fold(seal_fold(s));
    return s >= SEAL_P ? s - SEAL_P : s;
}

} // namespace fhe
