// seal_check.hpp -- the seal of a row at rest: two position-weighted sums modulo the Mersenne prime p = 2^61 - 1, and the third sum
// that turns it into a single-error-correcting code (host + device: the kernels of seal_checked.hip and seal_repair.hip and the CPU
// emulations tests/emu/emu_seal_check.cpp and tests/emu/emu_seal_repair.cpp compile the same functions).
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
#include <type_traits>

#include "modarith.hpp"

namespace fhe {

// f(integral_constant<int, I>) for I = B .. N - 1, unrolled by the template and not by the optimiser: an accumulator indexed by I
// is then indexed by a constant whatever the size of the loop body, and never leaves the registers
template <int B, int N, class F> FHE_HD void seal_each(F &&f)
{
    if constexpr (B < N) {
        f(std::integral_constant<int, B>{});
        seal_each<B + 1, N>(f);
    }
}

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

// the two running sums, each at most p + 7 between calls.  WORDS, get(i) and merge(const u64 *) are what every accumulator shows
// to the combine of seal_sweep.hpp: its sums as they travel (shuffles, LDS, a job's partials in memory), in the partials' order
struct SealAcc {
    static constexpr int WORDS = 2;
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
    FHE_HD u64 get(int i) const { return i ? s1 : s0; }
    FHE_HD void merge(const u64 *o) { merge(o[0], o[1]); }
};

// a lazily reduced sum -> [0, p): two folds bring any 64-bit value to at most p, and p itself is 0
FHE_HD u64 seal_canonical(u64 s)
{
    s = seal_fold(seal_fold(s));
    return s >= SEAL_P ? s - SEAL_P : s;
}

// what a finish step decides for one row: s0 / s1 = its lazily reduced digests, stored = the seal as it lies in memory.  True where
// the row raises SEAL_SUM; a stored sum is held word for word, so one that is not canonical counts as moved (seal_decide)
FHE_HD bool seal_differs(u64 s0, u64 s1, const u64 *stored) { return seal_canonical(s0) != stored[0] || seal_canonical(s1) != stored[1]; }

// what one lane (one chunk, one row) of a fused sweep has digested of N operand rows it reads side by side (the diagonals of
// BSGS inner sum, the key rows of the key switch: mac_seal.hpp): the two sums of each and the window bits
template <int N> struct SealRows {
    static constexpr int WORDS = 2 * N;
    SealAcc acc[N];
    u32 range = 0;      // bit r: a word of row r was >= q
    FHE_HD u64 get(int i) const { return acc[i >> 1].get(i & 1); }
    FHE_HD void merge(const u64 *o)
    {
        seal_each<0, N>([&](auto rc) {
            constexpr int r = decltype(rc)::value;
            acc[r].merge(o[2 * r], o[2 * r + 1]);
        });
    }
};

// ---- repair: a third sum locates and corrects one corrupted word per row (seal_repair.hip, capi_seal.cpp) ----
// Beside the seal {S0, S1} a row may carry the locator sum S2 = sum_j (j + 1)^2 x_j mod p.  With syndromes D_i = S_i' - S_i (the
// sums of the row as it is now, minus the stored ones) a change d in ONE word j gives D0 = d, D1 = w d, D2 = w^2 d with w = j + 1:
// w = D1 / D0 names the word and x = x' - d restores it exactly, because x < q < p.  Two sums alone would be unsafe: the same bit
// set in words j1, j2 with j1 + j2 even gives D1 / D0 = the midpoint's weight, in range, and an intact word would be "corrected"
// into a row that passes its seal.  For TWO changed words D1^2 - D0 D2 = -d1 d2 (w1 - w2)^2, every factor non-zero and below p, so
// the consistency test D1^2 = D0 D2 fails with certainty; a single-word change always passes it.  Three or more changed words
// pass it with probability about N / p per row on random data.

// outcome of a repair, per row (FHE_SEAL_* of include/fhe_mi355x.h)
enum { SEAL_CLEAN = 0, SEAL_REPAIRED = 1, SEAL_UNCORRECTABLE = 2, SEAL_TRANSIENT = 3, SEAL_SUSPECT = 4 };

// chunks per row, as a shift
FHE_HD int seal_log_chunks(int logn) { return logn > SEAL_LOG_CHUNK ? logn - SEAL_LOG_CHUNK : 0; }

// a b mod p, canonical, for canonical a, b < p: the 122-bit product is hi 2^64 + lo with hi < 2^58, and 2^64 = 8 modulo p
FHE_HD u64 seal_mulmod(u64 a, u64 b) { return seal_canonical((mulhi64(a, b) << 3) + seal_fold(a * b)); }

// a^(p - 2) mod p: the inverse of a canonical a != 0 (0 for a = 0).  p - 2 = 2^61 - 3 has every bit below 61 set except bit 1
FHE_HD u64 seal_inv(u64 a)
{
    u64 r = 1;
    for (int b = 60; b >= 0; b--) {
        r = seal_mulmod(r, r);
        if (b != 1) r = seal_mulmod(r, a);
    }
    return r;
}

// w^2 x mod p, lazily, for a folded x and the 32-bit weight w = j + 1: the square passes 2^32 from N = 2^17 on, so the weight is
// applied twice and the square is never formed
FHE_HD u64 seal_w2mul(u64 x, u32 w) { return seal_wmul(seal_fold(seal_wmul(x, w)), w); }

// the three running sums, each at most p + 7 between calls
struct SealAcc3 : SealAcc {
    u64 s2 = 0;
    FHE_HD void add(u64 x, u32 j)
    {
        const u64 f = seal_fold(x);
        const u64 t = seal_wmul(f, j + 1);
        s0 = seal_fold(s0 + f);
        s1 = seal_fold(s1 + t);
        s2 = seal_fold(s2 + seal_wmul(seal_fold(t), j + 1));
    }
    FHE_HD void merge(u64 o0, u64 o1, u64 o2)
    {
        SealAcc::merge(o0, o1);
        s2 = seal_fold(s2 + seal_fold(o2));
    }
};

// a - b mod p, canonical, for canonical a, b
FHE_HD u64 seal_submod(u64 a, u64 b) { return seal_canonical(a + SEAL_P - b); }

// the index j of a single-word change with canonical syndromes D0 != 0, D1, D2 in a row of n words, or -1 ("none")
FHE_HD long long seal_locate(u64 d0, u64 d1, u64 d2, u32 n)
{
    if (d0 == 0) return -1;
    if (seal_mulmod(d1, d1) != seal_mulmod(d0, d2)) return -1;
    const u64 w = seal_mulmod(d1, seal_inv(d0));
    if (w < 1 || w > n) return -1;
    if (d2 != seal_mulmod(w, d1)) return -1;
    return (long long)w - 1;
}

// the word x' of now with the change D0 taken back: canonical(fold(x') - D0) mod p, the original word where it was below p
FHE_HD u64 seal_restore(u64 x_now, u64 d0) { return seal_canonical(seal_fold(x_now) + SEAL_P - d0); }

// what one lane decides for a flagged row from a fresh sweep: got = the row's three canonical sums as it is now, stored = {S0, S1
// of the seal, S2 of the locator} as they lie in memory, n_out = how many words are >= q and out_idx the index of one of them.
// A stored sum is held against the fresh one word for word, so a stored value that is not canonical counts as moved.
//   status SEAL_TRANSIENT    every sum equal, every word in the window: the first sweep saw something memory does not hold
//          SEAL_SUSPECT      exactly one sum moved and every word in the window: the stored sum is the likely casualty
//          SEAL_REPAIRED     a candidate: word `index` is to become seal_restore(x'[index], d0) -- provided that is below q
//                            (seal_repair_word) and a second sweep confirms the row
//          SEAL_UNCORRECTABLE anything else
struct SealVerdict {
    int status;
    u32 index;
    u64 d0;
};
FHE_HD SealVerdict seal_decide(const u64 got[3], const u64 stored[3], u32 n_out, u32 out_idx, u32 n)
{
    const int moved = (got[0] != stored[0]) + (got[1] != stored[1]) + (got[2] != stored[2]);
    if (moved == 0) {
        if (n_out == 0) return SealVerdict{SEAL_TRANSIENT, 0, 0};
        // x' = x + k p: invisible to every sum, seen by the window alone
        return n_out == 1 ? SealVerdict{SEAL_REPAIRED, out_idx, 0} : SealVerdict{SEAL_UNCORRECTABLE, 0, 0};
    }
    if (moved == 1) return SealVerdict{n_out == 0 ? SEAL_SUSPECT : SEAL_UNCORRECTABLE, 0, 0};
    if (stored[0] >= SEAL_P || stored[1] >= SEAL_P || stored[2] >= SEAL_P) return SealVerdict{SEAL_UNCORRECTABLE, 0, 0};
    const u64 d0 = seal_submod(got[0], stored[0]);
    const long long j = seal_locate(d0, seal_submod(got[1], stored[1]), seal_submod(got[2], stored[2]), n);
    if (j < 0 || n_out > 1 || (n_out == 1 && out_idx != (u32)j)) return SealVerdict{SEAL_UNCORRECTABLE, 0, 0};
    return SealVerdict{SEAL_REPAIRED, (u32)j, d0};
}

// the restored word of a SEAL_REPAIRED candidate, or false where it would not be below q (the row is then left alone)
FHE_HD bool seal_repair_word(u64 x_now, u64 d0, u64 q, u64 &restored)
{
    restored = seal_restore(x_now, d0);
    return restored < q;
}

} // namespace fhe
