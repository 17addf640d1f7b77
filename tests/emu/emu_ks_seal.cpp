// emu_ks_seal.cpp -- CPU emulation of the sealed key-switch inner product (TEST INFRASTRUCTURE ONLY).
//
// Compiles fhe_reliability_gpu_amd/csrc/ks_seal.hpp -- the per-pair step and the per-row decision the kernels of
// keyswitch_sealed.hip call -- with g++ and runs one row's job loop the way k_ks_mac_sealed runs it (chunks of 2^log_chunk words,
// `lanes` lanes of two adjacent words per step, the d loop unrolled to the band ND, the butterfly of the wave shuffles, the waves,
// then the chunks' partials [2 dnum][2], in either order) followed by k_ks_seal_finish's decision per key row, so that words, digests
// and flag bits can be checked against Python integers without a GPU.  The library never links this file.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I<csrc> emu_ks_seal.cpp -o libemu_ks_seal.so
#include "ks_seal.hpp"

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

struct Row {
    const u64 *c, *ext, *key;      // [n], [dnum][n], [dnum][2][n]
    u32 n, dnum;
    int own;                       // the digit whose own limb range holds this row (x from c), or -1 (x from ext everywhere)
};

template <class D, int ND>
void sealed_row(const Row &r, const LimbParams &p, u32 words, u32 lanes, bool reverse, const u64 *seal, const KsHit &hit, u64 *acc0, u64 *acc1, u32 *fl,
                u64 *digest, u32 *seal_flags)
{
    const PwFault none[2] = {{-1, 0}, {-1, 0}};
    const u32 R = 2 * r.dnum;
    std::vector<SealAcc> row(R);
    u32 range = 0;
    fl[0] = fl[1] = 0;
    const u32 chunks = r.n / words;
    for (u32 ci = 0; ci < chunks; ci++) {
        const u32 i0 = (reverse ? chunks - 1 - ci : ci) * words;
        std::vector<KsSeal<ND>> cur(lanes);
        for (u32 t = 0; t < lanes; t++)
            for (u32 s = 2 * t; s < words; s += 2 * lanes) {
                const u32 i = i0 + s;
                auto ld = [&](u32 d, u64 *x, u64 *k0, u64 *k1) {
                    const u64 *src = (int)d == r.own ? r.c : r.ext + (size_t)d * r.n;
                    const u64 *key = r.key + (size_t)d * 2 * r.n;
                    for (int w = 0; w < 2; w++) x[w] = src[i + w], k0[w] = key[i + w], k1[w] = key[r.n + i + w];
                };
                u64 c0[2], c1[2];
                ks_seal_pair<D, ND, true>(cur[t], r.dnum, i, p, ld, hit, none, none, c0, c1, fl[0], fl[1]);
                for (int w = 0; w < 2; w++) acc0[i + w] = c0[w], acc1[i + w] = c1[w];
            }
        const u32 wave = lanes < 64 ? lanes : 64;
        for (u32 o = wave / 2; o; o >>= 1) {      // __shfl_xor inside each wave
            std::vector<KsSeal<ND>> next = cur;
            for (u32 t = 0; t < lanes; t++) {
                for (u32 a = 0; a < 2 * ND; a++) next[t].acc[a].merge(cur[t ^ o].acc[a].s0, cur[t ^ o].acc[a].s1);
                next[t].range |= cur[t ^ o].range;
            }
            cur = next;
        }
        KsSeal<ND> part = cur[0];
        for (u32 w = 1; w < lanes / wave; w++) {
            for (u32 a = 0; a < 2 * ND; a++) part.acc[a].merge(cur[wave * w].acc[a].s0, cur[wave * w].acc[a].s1);
            part.range |= cur[wave * w].range;
        }
        // the chunk's partial as it lies in memory ([2 dnum][2]), then k_ks_seal_finish's sum over the chunks
        for (u32 a = 0; a < R; a++) row[a].merge(part.acc[a].s0, part.acc[a].s1);
        range |= part.range;
    }
    for (u32 a = 0; a < R; a++) {
        digest[2 * a] = seal_canonical(row[a].s0);
        digest[2 * a + 1] = seal_canonical(row[a].s1);
        seal_flags[a] = (range >> a & 1 ? (u32)SEAL_RANGE : 0u) | (ks_seal_decide(row[a].s0, row[a].s1, seal + 2 * a) ? (u32)SEAL_SUM : 0u);
    }
}

template <int ND>
void sealed_row_on(const Row &r, const LimbParams &p, u32 words, u32 lanes, bool reverse, const u64 *seal, const KsHit &hit, u64 *acc0, u64 *acc1, u32 *fl,
                   u64 *digest, u32 *seal_flags)
{
    if (p.path == PATH_F64) sealed_row<KsDotF64, ND>(r, p, words, lanes, reverse, seal, hit, acc0, acc1, fl, digest, seal_flags);
    else sealed_row<KsDotU64, ND>(r, p, words, lanes, reverse, seal, hit, acc0, acc1, fl, digest, seal_flags);
}

} // namespace

extern "C" {

unsigned emu_ks_seal_max_dnum() { return KS_SEAL_MAX_DNUM; }

// One row of n words (n a multiple of 2^log_chunk >= 2) of a key switch with dnum digits: c = the row of the input, ext = [dnum][n]
// the digits' extensions, own = the digit that takes its words from c (-1: none), key = [dnum][2][n] the key's words on this row,
// seal = [2 dnum][2] their stored seals (key row 2 d + h); path 0 = FP64-term form, 1 = U64; nd = the instantiated band (2, 4, 8,
// 12; >= dnum); lanes = a power of two, the lanes of a workgroup (256 on the device); reverse: the chunks' partials merge last
// chunk first.  hit_dh >= 0: bit hit_bit of word hit_coeff of key row hit_dh = 2 d + h is flipped in the register as loaded.
// Out: acc0, acc1 = the words of both halves, fl[2] = the OR of each half's residue flags, digest = [2 dnum][2] canonical sums of
// the key rows as loaded, seal_flags = [2 dnum]
int emu_ks_sealed(const u64 *c, const u64 *ext, const u64 *key, u32 n, u32 dnum, int own, u64 q, int path, int nd, int log_chunk, u32 lanes, int reverse,
                  const u64 *seal, int hit_dh, u32 hit_coeff, int hit_bit, u64 *acc0, u64 *acc1, u32 *fl, u64 *digest, u32 *seal_flags)
{
    if ((path == PATH_F64 && q >= ((u64)1 << 50)) || log_chunk < 1 || n % (1u << log_chunk) || !lanes || (lanes & (lanes - 1)) || dnum < 1 || dnum > (u32)nd) return -1;
    const LimbParams p = limb(q, path);
    const Row r{c, ext, key, n, dnum, own};
    const KsHit hit = hit_dh >= 0 ? KsHit{(u32)hit_dh / 2, (u32)hit_dh % 2, hit_coeff, (u64)1 << hit_bit} : KsHit{0xFFFFFFFFu, 0, 0, 0};
    const u32 words = 1u << log_chunk;
    switch (nd) {
    case 2: sealed_row_on<2>(r, p, words, lanes, reverse != 0, seal, hit, acc0, acc1, fl, digest, seal_flags); break;
    case 4: sealed_row_on<4>(r, p, words, lanes, reverse != 0, seal, hit, acc0, acc1, fl, digest, seal_flags); break;
    case 8: sealed_row_on<8>(r, p, words, lanes, reverse != 0, seal, hit, acc0, acc1, fl, digest, seal_flags); break;
    case 12: sealed_row_on<12>(r, p, words, lanes, reverse != 0, seal, hit, acc0, acc1, fl, digest, seal_flags); break;
    default: return -1;
    }
    return 0;
}

} // extern "C"
