// emu_tensor_seal.cpp -- CPU emulation of the sealed tensor product (TEST INFRASTRUCTURE ONLY).
//
// Compiles fhe_reliability_gpu_amd/csrc/tensor_seal.hpp -- the per-word step and the per-row decision the kernels of
// tensor_sealed.hip call -- with g++ and runs one row's job loop the way k_tensor_sealed runs it (chunks of 2^log_chunk words,
// `lanes` lanes of two adjacent words per step, the butterfly of the wave shuffles, the waves, then the chunks' partials, in either
// order) followed by k_tensor_seal_finish's decision per operand, so that words, digests and flag bits can be checked against
// Python integers without a GPU.  The library never links this file.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I<csrc> emu_tensor_seal.cpp -o libemu_tensor_seal.so
#include "tensor_seal.hpp"

#include <vector>

using namespace fhe;

namespace {

// the limb constants as capi.cpp build_tables fills them (the fields these elements read)
LimbParams limb(u64 q, int path)
{
    LimbParams p{};
    p.q = q;
    p.two_q = 2 * q;
    p.n = (double)q;
    p.ninv = 1.0 / p.n;
    const unsigned __int128 ratio = ~(unsigned __int128)0 / q;      // floor(2^128 / q) for q not a power of two
    p.barrett_lo = (u64)ratio;
    p.barrett_hi = (u64)(ratio >> 64);
    p.path = path;
    return p;
}

template <bool OUT>
void sealed_row(const u64 *const *ops, u32 n, const LimbParams &p, u32 words, u32 lanes, bool reverse, const u64 *seal, int hit_op, u32 hit_coeff, u64 hit_mask,
                u64 *const *d, u32 *fl, u64 *digest, u32 *seal_flags)
{
    constexpr int W = TensorSealAcc<OUT>::WORDS;
    const PwFault none{-1, 0};
    TensorSealAcc<OUT> row;
    u32 bad = 0;
    fl[0] = fl[1] = fl[2] = 0;
    const u32 chunks = n / words;
    for (u32 c = 0; c < chunks; c++) {
        const u32 j0 = (reverse ? chunks - 1 - c : c) * words;
        std::vector<TensorSealAcc<OUT>> cur(lanes);
        for (u32 t = 0; t < lanes; t++)
            for (u32 i = 2 * t; i < words; i += 2 * lanes)
                for (u32 j = j0 + i; j < j0 + i + 2; j++) {
                    const u64 x[4] = {ops[0][j], ops[1][j], ops[2][j], ops[3][j]};
                    const TensorHit hit{hit_op, hit_op >= 0 && j == hit_coeff ? hit_mask : 0};
                    u64 w[3];
                    u32 f[3];
                    cur[t].step(x, j, p, hit, none, w, f, bad);
                    for (int k = 0; k < 3; k++) d[k][j] = w[k], fl[k] |= f[k];
                }
        const u32 wave = lanes < 64 ? lanes : 64;
        for (u32 o = wave / 2; o; o >>= 1) {      // __shfl_xor inside each wave
            std::vector<TensorSealAcc<OUT>> next = cur;
            for (u32 t = 0; t < lanes; t++) {
                u64 other[W];
                for (int i = 0; i < W; i++) other[i] = cur[t ^ o].get(i);
                next[t].merge(other);
            }
            cur = next;
        }
        TensorSealAcc<OUT> part = cur[0];
        for (u32 w = 1; w < lanes / wave; w++) {
            u64 other[W];
            for (int i = 0; i < W; i++) other[i] = cur[wave * w].get(i);
            part.merge(other);
        }
        // the chunk's partial as it lies in memory, then k_tensor_seal_finish's sum over the chunks
        u64 stored[W];
        for (int i = 0; i < W; i++) stored[i] = part.get(i);
        row.merge(stored);
    }
    for (int i = 0; i < TensorSealAcc<OUT>::ACCS; i++) {
        digest[2 * i] = seal_canonical(row.s[i].s0);
        digest[2 * i + 1] = seal_canonical(row.s[i].s1);
    }
    for (int o = 0; o < 4; o++)
        seal_flags[o] = (bad >> o & 1 ? (u32)SEAL_RANGE : 0u) | (tensor_seal_decide(row.s[o].s0, row.s[o].s1, seal + 2 * o) ? (u32)SEAL_SUM : 0u);
}

} // namespace

extern "C" {

// One row of n words (n a multiple of 2^log_chunk >= 2): a0, a1, b0, b1 = the operand rows, seal = [4][2] their stored seals;
// path 0 = FP64-term form, 1 = U64; lanes = a power of two, the lanes of a workgroup (256 on the device); reverse: the chunks'
// partials merge last chunk first.  hit_op >= 0: bit hit_bit of word hit_coeff of that operand is flipped in the register as
// loaded.  Out: d0, d1, d2 = the words, fl[3] = the OR of each part's residue flags, digest = [7][2] (out) or [4][2] canonical
// sums of the rows as loaded (and of the words as stored), seal_flags = [4]
int emu_tensor_sealed(const u64 *a0, const u64 *a1, const u64 *b0, const u64 *b1, u32 n, u64 q, int path, int log_chunk, u32 lanes, int reverse, int out,
                      const u64 *seal, int hit_op, u32 hit_coeff, int hit_bit, u64 *d0, u64 *d1, u64 *d2, u32 *fl, u64 *digest, u32 *seal_flags)
{
    if ((path == PATH_F64 && q >= ((u64)1 << 50)) || log_chunk < 1 || n % (1u << log_chunk) || !lanes || (lanes & (lanes - 1))) return -1;
    const LimbParams p = limb(q, path);
    const u64 *ops[4] = {a0, a1, b0, b1};
    u64 *d[3] = {d0, d1, d2};
    const u64 mask = hit_bit >= 0 ? (u64)1 << hit_bit : 0;
    if (out) sealed_row<true>(ops, n, p, 1u << log_chunk, lanes, reverse != 0, seal, hit_op, hit_coeff, mask, d, fl, digest, seal_flags);
    else sealed_row<false>(ops, n, p, 1u << log_chunk, lanes, reverse != 0, seal, hit_op, hit_coeff, mask, d, fl, digest, seal_flags);
    return 0;
}

} // extern "C"
