// galois_check.hpp -- the checked NTT-domain Galois permutation (host + device: the kernel of galois_checked.hip and the CPU
// emulation in tests/emu/emu_galois_check.cpp compile the same functions).
//
// For one unit (a row of N words in the transform's bit-reversed slot order) the permutation writes dst[j] = src[pi_k(j)], pi_k =
// galois_slot(., logn, k) of ntt_core.hpp (the slot map of k_automorphism_ntt).  A permutation moves words and computes nothing, so
// there is no arithmetic identity per word; what is checked is one position-weighted sum per unit, modulo m = 2^32 - 1 with the
// lane arithmetic of residue_check.hpp (r(x) = x mod m, w(j) = j + 1):
//     S_out = sum_j  w(j)           r(word stored at j)
//     S_in  = sum_i  w(pi_kinv(i))  r(src[i])                  kinv = k^-1 mod 2N
// pi_kinv is the inverse permutation of pi_k (both are multiplications of the odd exponent 2 bitrev(j) + 1 modulo 2N), so the
// two sums have the same terms in another order on a clean run.  The two sides share nothing but src itself: S_out takes the
// register about to be stored and the destination index; S_in comes from a second, LINEAR read of src (position i reads src[i])
// and finds its weight through the index formula evaluated with kinv, which the host computes (host::inv_mod).  Neither the
// gathered register nor the gather's index computation feeds S_in.  Every term is below 2^32 (res_mul), a unit has at most 2^30
// of them, so plain 64-bit sums cannot overflow; integer addition is associative, so the order in which partial sums meet does
// not matter and the result is deterministic.  The sums are folded (res64) and compared once per unit.
//
// Coverage: a single-bit flip of a moved word (bit b, either half of the word) shifts S_out by +-w 2^(b mod 32); gcd(2^b, m) = 1
// and 0 < w(j) <= N < m, so it is always caught.  A wrong source index that fetches x' instead of x is caught unless
// w(j) (r(x') - r(x)) = 0 (mod m): on random words with probability at most gcd(w(j), m) / m <= N / m.  Not covered: a wrong
// galois_elt handed in by the caller (both sides follow it), faults already in src, a word corrupted in memory after the store.
//
// Injection points of the test hook (one shot, one (unit, coefficient)): GAL_AT_WORD = the gathered word before it is stored and
// summed, any of its 64 bits; GAL_AT_INDEX = the gather's source index, a bit below log N (so the wrong index stays in the row).
#pragma once
#include "ntt_core.hpp"
#include "residue_check.hpp"

namespace fhe {

enum { GAL_AT_WORD = 0, GAL_AT_INDEX = 1 };
struct GaloisFault {
    int point = -1;      // < 0: none
    u32 unit = 0;
    u64 coeff = 0;
    int bit = 0;
};
FHE_HD bool galois_point_exists(int point, int bit, int logn) { return point == GAL_AT_WORD ? bit >= 0 && bit < 64 : point == GAL_AT_INDEX && bit >= 0 && bit < logn; }

FHE_HD u32 galois_weight(u32 j) { return j + 1; }

// destination side of slot j: the word to store at row[j] and its term of S_out.  word_mask / index_mask: the test hook (0 on
// every element but the armed one)
FHE_HD u64 galois_gather(const u64 *src_row, u32 j, int logn, u32 k, u64 word_mask, u32 index_mask, u64 &out_term)
{
    const u32 from = galois_slot(j, logn, k) ^ index_mask;
    const u64 v = src_row[from] ^ word_mask;
    out_term = res_mul(galois_weight(j), res64(v));
    return v;
}

// source side of slot i: the term of S_in of the word x = src_row[i] read in place; its weight is the slot pi_kinv(i) the word goes to
FHE_HD u64 galois_source_term(u64 x, u32 i, int logn, u32 kinv) { return res_mul(galois_weight(galois_slot(i, logn, kinv)), res64(x)); }

FHE_HD u32 galois_sums_flag(u64 s_in, u64 s_out) { return res_eq(res64(s_in), res64(s_out)) ? 0u : 1u; }

} // namespace fhe
