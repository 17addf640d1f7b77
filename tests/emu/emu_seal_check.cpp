// emu_seal_check.cpp -- CPU emulation of the row seals (TEST INFRASTRUCTURE ONLY).
//
// Compiles fhe_reliability_gpu_amd/csrc/seal_check.hpp -- the functions the kernels of seal_checked.hip call -- with g++ and runs
// them over rows of words, once as a single sweep in index order and once cut the way k_row_digest cuts a row (chunks, 256 lanes of
// two adjacent words per load, the butterfly of the wave shuffles, the waves, then the chunks' partials), so that seals and flag
// bits can be checked against Python integers without a GPU.  residue_check.hpp's fold modulo 2^32 - 1 is exported next to it, for
// the changes it cannot see.  The library never links this file.
//
//   g++ -O2 -std=c++17 -shared -fPIC -I<csrc> emu_seal_check.cpp -o libemu_seal_check.so
#include "residue_check.hpp"
#include "seal_check.hpp"

using namespace fhe;

namespace {

SealAcc sweep(const u64 *x, size_t n)
{
    SealAcc a;
    for (size_t j = 0; j < n; j++) a.add(x[j], (u32)j);
    return a;
}

// one chunk of `words` words starting at row index j0, as a workgroup of 256 lanes sums it
SealAcc chunk_as_workgroup(const u64 *row, u32 j0, u32 words)
{
    SealAcc lane[256];
    for (u32 t = 0; t < 256; t++)
        for (u32 i = 2 * t; i < words; i += 512) {
            lane[t].add(row[j0 + i], j0 + i);
            lane[t].add(row[j0 + i + 1], j0 + i + 1);
        }
    for (u32 o = 32; o; o >>= 1) {      // __shfl_xor inside each wave of 64
        SealAcc next[256];
        for (u32 t = 0; t < 256; t++) {
            next[t] = lane[t];
            next[t].merge(lane[t ^ o].s0, lane[t ^ o].s1);
        }
        for (u32 t = 0; t < 256; t++) lane[t] = next[t];
    }
    SealAcc a = lane[0];
    for (u32 w = 1; w < 4; w++) a.merge(lane[64 * w].s0, lane[64 * w].s1);
    return a;
}

} // namespace

extern "C" {

// seal[r] = {S0, S1} of row r of x = [rows][n], one sweep in index order
void emu_seal(const u64 *x, size_t rows, size_t n, u64 *seal)
{
    for (size_t r = 0; r < rows; r++) {
        const SealAcc a = sweep(x + r * n, n);
        seal[2 * r] = seal_canonical(a.s0);
        seal[2 * r + 1] = seal_canonical(a.s1);
    }
}

// the same from chunks of 2^log_chunk words (n a multiple), each summed as a workgroup sums it, the partials merged last chunk first
void emu_seal_chunked(const u64 *x, size_t rows, size_t n, int log_chunk, u64 *seal)
{
    const u32 words = 1u << log_chunk;
    for (size_t r = 0; r < rows; r++) {
        SealAcc a;
        for (size_t c = n / words; c-- > 0;) {
            const SealAcc part = chunk_as_workgroup(x + r * n, (u32)(c * words), words);
            a.merge(part.s0, part.s1);
        }
        seal[2 * r] = seal_canonical(a.s0);
        seal[2 * r + 1] = seal_canonical(a.s1);
    }
}

// flags[r] = SEAL_SUM where row r's sums differ from seal[r], SEAL_RANGE where a word is >= q
void emu_seal_verify(const u64 *x, size_t rows, size_t n, u64 q, const u64 *seal, u32 *flags)
{
    for (size_t r = 0; r < rows; r++) {
        const SealAcc a = sweep(x + r * n, n);
        u32 f = seal_canonical(a.s0) != seal[2 * r] || seal_canonical(a.s1) != seal[2 * r + 1] ? (u32)SEAL_SUM : 0u;
        for (size_t j = 0; j < n; j++)
            if (x[r * n + j] >= q) f |= (u32)SEAL_RANGE;
        flags[r] = f;
    }
}

u64 emu_seal_canonical(u64 s) { return seal_canonical(s); }

// residue_check.hpp: are x and y the same modulo 2^32 - 1, as the checked products see them
int emu_fold32_equal(u64 x, u64 y) { return res_eq(res64(x), res64(y)) ? 1 : 0; }

} // extern "C"
