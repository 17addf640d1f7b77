// tensor_seal.hpp -- the tensor product with its operands verified on the load that multiplies them, and its results digested from
// the registers that are stored (host + device: the kernels of tensor_sealed.hip and the CPU emulation tests/emu/emu_tensor_seal.cpp
// compile the same functions).
//
// fhe_hmult_sealed verifies a0, a1, b0, b1 by four sweeps and then runs k_tensor_checked, which loads the four operands a second
// time: a word that is wrong on that second load only passes the seal, is a consistent operand to the residue identity of
// residue_check.hpp, and gives a wrong product with no flag.  The tensor product reads every operand word exactly once, so the seal
// of seal_check.hpp (S0 = sum x_j, S1 = sum (j + 1) x_j modulo p = 2^61 - 1, and the window x_j < q) is digested from the very
// register that is then handed to the product: no second sweep, and the verified load IS the consuming load.  With OUT the three
// result words are digested from the registers about to be stored, so a three-part ciphertext leaves the call sealed without three
// more sweeps; a fault after that digest (the store, memory) is the next verification's to catch.
//
// The arithmetic is k_tensor_checked's, unchanged: checked_dot<1> for d0, checked_dot<2> over {a0, a1} . {b1, b0} for d1,
// checked_dot<1> for d2, FP64 terms where the limb's path is PATH_F64 and Barrett elsewhere, the pointwise test fault on the d1 sum
// only.  The words are fhe_tensor_product's bit for bit -- also for an operand word that is not canonical: the call flags such a
// word (the window bit here, PW_OPERAND in the residue flags), it does not fix it.
//
// What a raised operand word means: SEAL_SUM -- the row as it was loaded for this product is not the row that was sealed (one or two
// changed words: with certainty, seal_check.hpp), or a stored sum is not canonical; SEAL_RANGE -- a loaded word is >= q_l.  Integer
// arithmetic modulo p throughout the digests: no sum depends on how a row is cut into chunks, lanes or waves, nor on the order in
// which partial sums are merged.
#pragma once
#include "residue_check.hpp"
#include "seal_check.hpp"

namespace fhe {

// operands in argument order, then the results
enum { TS_A0 = 0, TS_A1 = 1, TS_B0 = 2, TS_B1 = 3, TS_D0 = 4 };

// the one-shot test fault of fhe_ctx_inject_fault_tensor_sealed as one word meets it: XOR mask into operand `op` in the register as
// loaded -- before the window, the digest and the product read it (mask == 0: not this word)
struct TensorHit {
    int op;
    u64 mask;
};

// what one lane (one chunk, one row) has digested: the two sums of each operand and, with OUT, of each result
template <bool OUT> struct TensorSealAcc {
    static constexpr int ACCS = OUT ? 7 : 4;
    static constexpr int WORDS = 2 * ACCS;      // {a0: s0, s1; a1; b0; b1; [d0; d1; d2]}: a job's partials
    SealAcc s[ACCS];

    // the four operand words at index j of their row, on arithmetic path D (KsDotU64 / KsDotF64): d = the words of d0, d1, d2,
    // fl = their residue flags, bad |= bit o where operand o is outside its window.  f = the pointwise test fault, of the d1 sum
    template <class D> FHE_HD void step_on(const u64 (&x)[4], u32 j, const LimbParams &p, const TensorHit &hit, const PwFault &f, u64 (&d)[3], u32 (&fl)[3], u32 &bad)
    {
        u64 v[4];
        for (int o = 0; o < 4; o++) {
            v[o] = hit.op == o ? x[o] ^ hit.mask : x[o];
            bad |= v[o] >= p.q ? 1u << o : 0u;
            s[o].add(v[o], j);
        }
        const u64 x0[1] = {v[TS_A0]}, y0[1] = {v[TS_B0]}, x2[1] = {v[TS_A1]}, y2[1] = {v[TS_B1]};
        const u64 x1[2] = {v[TS_A0], v[TS_A1]}, y1[2] = {v[TS_B1], v[TS_B0]};
        const PwFault none{-1, 0};
        d[0] = checked_dot<D, 1>(x0, y0, p, fl[0], none);
        d[1] = checked_dot<D, 2>(x1, y1, p, fl[1], f);
        d[2] = checked_dot<D, 1>(x2, y2, p, fl[2], none);
        if constexpr (OUT)
            for (int i = 0; i < 3; i++) s[TS_D0 + i].add(d[i], j);
    }
    // the same on the limb's own path (checked_dot_f64 / checked_dot_u64, as k_tensor_checked chooses)
    FHE_HD void step(const u64 (&x)[4], u32 j, const LimbParams &p, const TensorHit &hit, const PwFault &f, u64 (&d)[3], u32 (&fl)[3], u32 &bad)
    {
        if (p.path == PATH_F64) step_on<KsDotF64>(x, j, p, hit, f, d, fl, bad);
        else step_on<KsDotU64>(x, j, p, hit, f, d, fl, bad);
    }

    // the sums as they travel (shuffles, LDS, the partials in memory): WORDS of them, in the order of a job's partials
    FHE_HD u64 get(int i) const { return i & 1 ? s[i >> 1].s1 : s[i >> 1].s0; }
    FHE_HD void merge(const u64 *o)
    {
        for (int i = 0; i < ACCS; i++) s[i].merge(o[2 * i], o[2 * i + 1]);
    }
};

// the name tests/emu/emu_tensor_seal.cpp knows the finish step's decision by
FHE_HD bool tensor_seal_decide(u64 s0, u64 s1, const u64 *stored) { return seal_differs(s0, s1, stored); }

} // namespace fhe
