// emu_subscale_seal.cpp -- CPU emulation of the sealed mod-down tail (TEST INFRASTRUCTURE ONLY).
//
// Compiles fhe_reliability_gpu_amd/csrc/subscale_seal.hpp -- the per-word step and the per-row verdict the kernels of
// subscale_sealed.hip call -- with g++ and runs one row's job loop the way k_sub_scale_sealed runs it (chunks of 2^log_chunk words,
// `lanes` lanes of two adjacent words per step, the butterfly of the wave shuffles, the waves, then the chunks' partials, in
// either order), so that words, digests and flag bits can be checked against Python integers without a GPU.  The library never
// links this file.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I<csrc> emu_subscale_seal.cpp -o libemu_subscale_seal.so
#include "subscale_seal.hpp"

#include <vector>

using namespace fhe;

namespace {

struct Consts {
    u64 q, r0, r1;
    u32 rq;
};
Consts consts(u64 q)
{
    const unsigned __int128 ratio = ~(unsigned __int128)0 / q;      // floor(2^128 / q) for q not a power of two
    return Consts{q, (u64)ratio, (u64)(ratio >> 64), res64(q)};
}

struct Row {
    const u64 *x, *y, *add;      // null: absent
    u32 n;
    u64 s;
};

template <bool IN, bool OUT>
void sealed_row(const Row &r, const Consts &c, u32 words, u32 lanes, bool reverse, int hit_point, u32 hit_coeff, u64 hit_mask, u64 *out, u32 *fl, u64 *digest, u32 *range)
{
    typedef SubScaleSealAcc<IN, OUT> Acc;
    constexpr int R = Acc::WORDS / 2;
    const PwFault none{-1, 0};
    Acc row;
    *fl = 0;
    const u32 chunks = r.n / words;
    for (u32 ci = 0; ci < chunks; ci++) {
        const u32 j0 = (reverse ? chunks - 1 - ci : ci) * words;
        std::vector<Acc> cur(lanes);
        for (u32 t = 0; t < lanes; t++)
            for (u32 i = 2 * t; i < words; i += 2 * lanes)
                for (u32 w = 0; w < 2; w++) {
                    const u32 j = j0 + i + w;
                    const SubScaleWord sw{r.x ? r.x[j] : 0, r.y ? r.y[j] : 0, r.add ? r.add[j] : 0, r.x != nullptr, r.y != nullptr, r.add != nullptr};
                    const SubScaleHit hit{hit_point, hit_point >= 0 && j == hit_coeff ? hit_mask : 0};
                    out[j] = sub_scale_seal_word<IN, OUT, true>(cur[t], sw, j, r.s, c.q, c.r0, c.r1, c.rq, *fl, none, hit);
                }
        const u32 wave = lanes < 64 ? lanes : 64;
        for (u32 o = wave / 2; o; o >>= 1) {      // __shfl_xor inside each wave
            std::vector<Acc> next = cur;
            for (u32 t = 0; t < lanes; t++) {
                for (int a = 0; a < R; a++) next[t].acc[a].merge(cur[t ^ o].acc[a].s0, cur[t ^ o].acc[a].s1);
                next[t].range |= cur[t ^ o].range;
            }
            cur = next;
        }
        Acc part = cur[0];
        for (u32 w = 1; w < lanes / wave; w++) {
            for (int a = 0; a < R; a++) part.acc[a].merge(cur[wave * w].acc[a].s0, cur[wave * w].acc[a].s1);
            part.range |= cur[wave * w].range;
        }
        // the chunk's partial as it lies in memory, then the finish kernel's sum over the chunks
        u64 mem[Acc::WORDS];
        for (int i = 0; i < Acc::WORDS; i++) mem[i] = part.get(i);
        row.merge(mem);
        row.range |= part.range;
    }
    for (int a = 0; a < R; a++) {
        digest[2 * a] = seal_canonical(row.acc[a].s0);
        digest[2 * a + 1] = seal_canonical(row.acc[a].s1);
    }
    *range = row.range;
}

} // namespace

extern "C" {

// One word through the sealed step (IN and OUT, no hook) and through checked_sub_scale itself: has = bit 0 x, bit 1 y, bit 2 add.
// out = {the step's word, its flags, checked_sub_scale's word, its flags}
void emu_subscale_word(u64 x, u64 y, u64 add, int has, u64 s, u64 q, u32 j, u64 *out)
{
    const Consts c = consts(q);
    const PwFault none{-1, 0};
    SubScaleSealAcc<true, true> g;
    u32 f0 = 0, f1 = 0;
    const SubScaleWord w{has & 1 ? x : 0, has & 2 ? y : 0, has & 4 ? add : 0, (has & 1) != 0, (has & 2) != 0, (has & 4) != 0};
    out[0] = sub_scale_seal_word<true, true, false>(g, w, j, s, q, c.r0, c.r1, c.rq, f0, none, SubScaleHit{-1, 0});
    out[1] = f0;
    out[2] = checked_sub_scale(w.x, w.has_x, w.y, w.has_y, s, w.add, w.has_add, q, c.r0, c.r1, c.rq, f1, none);
    out[3] = f1;
}

// One row of n words (n a multiple of 2^log_chunk >= 2): x, y, add = the operands (null: absent), s the row's constant; form: bit 0
// IN, bit 1 OUT; lanes = a power of two (256 on the device); reverse: the chunks' partials merge last chunk first.  hit_point >= 0:
// bit hit_bit of word hit_coeff is flipped at that point (SS_AT_*).  Out: out = the words as stored, fl = the OR of the residue
// flags, digest = the canonical sums {x row as loaded (IN)}{out row as digested (OUT)}, range = a loaded x word was >= q
int emu_subscale_row(const u64 *x, const u64 *y, const u64 *add, u32 n, u64 s, u64 q, int form, int log_chunk, u32 lanes, int reverse, int hit_point, u32 hit_coeff,
                     int hit_bit, u64 *out, u32 *fl, u64 *digest, u32 *range)
{
    if (log_chunk < 1 || n % (1u << log_chunk) || !lanes || (lanes & (lanes - 1)) || ((form & 1) && !x)) return -1;
    const Consts c = consts(q);
    const Row r{x, y, add, n, s};
    const u32 words = 1u << log_chunk;
    const u64 mask = (u64)1 << hit_bit;
    switch (form) {
    case 3: sealed_row<true, true>(r, c, words, lanes, reverse != 0, hit_point, hit_coeff, mask, out, fl, digest, range); break;
    case 2: sealed_row<false, true>(r, c, words, lanes, reverse != 0, hit_point, hit_coeff, mask, out, fl, digest, range); break;
    case 1: sealed_row<true, false>(r, c, words, lanes, reverse != 0, hit_point, hit_coeff, mask, out, fl, digest, range); break;
    default: return -1;
    }
    return 0;
}

// the finish step's verdict on the x row: digest = its canonical sums, stored = its seal (null: not compared)
unsigned emu_subscale_verdict(const u64 *digest, int range, const u64 *stored) { return sub_scale_seal_verdict(digest[0], digest[1], range != 0, stored); }

int emu_subscale_point_exists(int point, int in, int out) { return sub_scale_seal_point_exists(point, in != 0, out != 0) ? 1 : 0; }

} // extern "C"
