// abft_taps.hpp -- the ABFT detector's observers of the transform passes ("taps", ntt_core.hpp): weighted checksums
// accumulated from the registers a pass has just loaded and from the words it is about to store, so that checking a
// transform costs arithmetic only, not extra sweeps over the data.  Compiles under hipcc and under g++ (tests/emu).
//
// Weights (capi_abft.cpp fhe_abft_create): w_i = (i mod 2^logp + 1) + (i div 2^logp + 1) (generate_weights,
// rfhe_framewk/src/negaclic_ntt.py:7-13), small integers made in registers on the FP64 path; w^ = F^-T w in the
// engine's bit-reversed order.  By linearity:
//   forward  X = F x           :  sum_i w_i x_i  ==  sum_j w^_j X_j
//   inverse  x = F^-1 X        :  sum_j w^_j X_j ==  sum_i w_i x_i         (the same two tables, sides swapped)
//   product  C_j = A_j B_j     :  sum_i w_i c_i  ==  sum_j w^_j A_j B_j    (c = F^-1 C)
//   natural-order (four-step) transform y = W x :  sum u x == sum m z == sum v y    (GsTap below)
// A fault between a tap's read of a register and the instruction that consumes the same register is not covered.
#pragma once
#include "ntt_plan.hpp"   // (NTT_THREADS)

namespace fhe {

// Checked forward transform: `in` on the words the first launch loads (weights w), `out` on the canonical words the last
// launch stores (weights w^).
template <class A, bool IN, bool OUT>
struct ChecksumTap {
    static constexpr bool ACTIVE = true;
    static constexpr bool MID = false;
    static constexpr bool STORES = false;
    typedef typename A::elem elem;
    TwPtr win, wout;                   // ArithU64: Shoup-encoded weights of this limb, offset to the tile's first element
    const u64 FHE_GLOBAL *wout8;       // ArithF64: output-side weights as plain residues (the quotient factor is one multiply)
    u32 pos0;                          // index of the tile's first element inside its limb
    int logp;                          // input-side weight of element i = (i mod 2^logp + 1) + (i div 2^logp + 1)
    elem acc_in, acc_out;
    int n_in, n_out;
    FHE_D void in(u32 idx, elem x, const typename A::Ctx &c)
    {
        if constexpr (IN) {
            if constexpr (A::PATH == PATH_F64) {
                // generate_weights (negaclic_ntt.py:7-13) computed in place of a table read: small integers
                const u32 i = pos0 + idx;
                // (the small integer becomes a double through the exponent trick of from_canonical: one subtraction, no v_cvt_f64_u32)
                const double w = ArithF64::from_canonical((u64)((i & ((1u << logp) - 1u)) + (i >> logp) + 2u));
                A::lazy_acc(acc_in, A::mulmod_w(x, w, w * c.ninv, c), ++n_in, c);
            } else {
                A::lazy_acc(acc_in, A::mulmod(x, win[idx], c), ++n_in, c);
            }
        }
    }
    FHE_D void out(u32 idx, u64 v, const typename A::Ctx &c)
    {
        if constexpr (OUT) {
            if constexpr (A::PATH == PATH_F64) {
                const double w = A::from_canonical(wout8[idx]);
                A::lazy_acc(acc_out, A::mulmod_w(A::from_canonical(v), w, w * c.ninv, c), ++n_out, c);
            } else {
                A::lazy_acc(acc_out, A::mulmod(A::from_canonical(v), wout[idx], c), ++n_out, c);
            }
        }
    }
};

// Checked inverse transform: the forward tap with the sides swapped -- `in` weighs the canonical words the first launch (the row
// pass) loads with w^ from the table, `out` weighs the canonical words the last launch (the column pass) stores with the
// register-generated w.  Same fields as ChecksumTap, so the kernels build either one from the same initialiser.
template <class A, bool IN, bool OUT>
struct InvChecksumTap {
    static constexpr bool ACTIVE = true;
    static constexpr bool MID = false;
    static constexpr bool STORES = false;
    typedef typename A::elem elem;
    TwPtr win, wout;
    const u64 FHE_GLOBAL *wout8;
    u32 pos0;
    int logp;
    elem acc_in, acc_out;
    int n_in, n_out;
    FHE_D void in(u32 idx, elem x, const typename A::Ctx &c)
    {
        if constexpr (IN) {
            if constexpr (A::PATH == PATH_F64) {
                const double w = A::from_canonical(wout8[idx]);
                A::lazy_acc(acc_in, A::mulmod_w(x, w, w * c.ninv, c), ++n_in, c);
            } else {
                A::lazy_acc(acc_in, A::mulmod(x, wout[idx], c), ++n_in, c);
            }
        }
    }
    FHE_D void out(u32 idx, u64 v, const typename A::Ctx &c)
    {
        if constexpr (OUT) {
            if constexpr (A::PATH == PATH_F64) {
                const u32 i = pos0 + idx;
                const double w = ArithF64::from_canonical((u64)((i & ((1u << logp) - 1u)) + (i >> logp) + 2u));
                A::lazy_acc(acc_out, A::mulmod_w(A::from_canonical(v), w, w * c.ninv, c), ++n_out, c);
            } else {
                A::lazy_acc(acc_out, A::mulmod(A::from_canonical(v), win[idx], c), ++n_out, c);
            }
        }
    }
};

// Per-phase detector (the reference checks its four-step flow phase by phase: batch_check of the column transforms,
// check_inter around the twiddle step, batch_check of the row transforms -- rfhe_framewk/src/ntt_test/relia_ntt_sim.cpp:235-292,
// 331-355; reliability_test/four_step_ntt_prot.py:185-194).  The engine's two launches ARE that flow -- column transforms,
// then row transforms with the twiddle folded into their butterflies -- so the checks sit at the same three places:
//   column pass :  sum_i w_i x_i  (words it loads)        ==  sum_i u_i y_i  (words it stores),   u = P1^-T w
//   hand-off    :  sum_i u_i y_i  (as stored)             ==  sum_i u_i y_i  (as loaded by the row pass)
//   row pass    :  sum_i u_i y_i  (words it loads)        ==  sum_j w^_j X_j (words it stores),   w^ = T^-T w
// PASS 0 = column pass (in: w, mid: u), PASS 1 = row pass (in: u, out: w^).
template <class A, int PASS>
struct PhaseTap {
    static constexpr bool ACTIVE = true;
    static constexpr bool MID = PASS == 0;
    static constexpr bool STORES = false;
    typedef typename A::elem elem;
    TwPtr win, umid, wout;             // ArithU64: Shoup-encoded weights of this limb, offset to the tile's first element
    const u64 FHE_GLOBAL *umid8, *wout8;   // ArithF64: the same weights as plain residues
    u32 pos0;
    int logp;
    elem acc_a, acc_b;
    int n_a, n_b;
    FHE_D void weigh(elem &acc, int &n, elem x, u32 idx, TwPtr tw, const u64 FHE_GLOBAL *tw8, const typename A::Ctx &c)
    {
        if constexpr (A::PATH == PATH_F64) {
            const double w = A::from_canonical(tw8[idx]);
            A::lazy_acc(acc, A::mulmod_w(x, w, w * c.ninv, c), ++n, c);
        } else {
            A::lazy_acc(acc, A::mulmod(x, tw[idx], c), ++n, c);
        }
    }
    FHE_D void in(u32 idx, elem x, const typename A::Ctx &c)
    {
        if constexpr (PASS == 0) {
            if constexpr (A::PATH == PATH_F64) {
                const u32 i = pos0 + idx;
                const double w = ArithF64::from_canonical((u64)((i & ((1u << logp) - 1u)) + (i >> logp) + 2u));     // generate_weights, negaclic_ntt.py:7-13
                A::lazy_acc(acc_a, A::mulmod_w(x, w, w * c.ninv, c), ++n_a, c);
            } else {
                A::lazy_acc(acc_a, A::mulmod(x, win[idx], c), ++n_a, c);
            }
        } else {
            weigh(acc_a, n_a, x, idx, umid, umid8, c);
        }
    }
    FHE_D void mid(u32 idx, elem x, const typename A::Ctx &c) { weigh(acc_b, n_b, x, idx, umid, umid8, c); }
    FHE_D void out(u32 idx, u64 v, const typename A::Ctx &c) { weigh(acc_b, n_b, A::from_canonical(v), idx, wout, wout8, c); }
};

// Checked natural-order transform (the four-step flow, reliability_test/four_step_ntt_prot.py:185-252: its two stages are checked
// with sum(C) == col_sums(A) . row_sums(B) and reported as stage1 / stage2).  y = W x, W[kappa][t] = omega^(kappa t), runs as the
// transposed network F^T of the forward one (F = R W, R the bit reversal): launch 1 = the gathering inverse row pass (RowPass
// ROWMODE 1), launch 2 = the inverse column pass; E1 = 2^S0 columns, E2 = 2^P points.  Weights (capi_fourstep_checked.cpp):
//   v  on the natural-order words launch 2 stores: v_kappa = (kappa mod 2^logp + 1) + (kappa div 2^logp + 1)  (generate_weights,
//      negaclic_ntt.py:7-13; the reference's all-ones weights would weigh x_0 only, W 1 = N delta_0);
//   u = W^T v = W v  on the words launch 1 gathers, at their NATURAL source index -- network position (local row, column k) of the
//      tile that starts at row0 holds src[brev_P(k) 2^S0 + row0 + row] (RowPass::gather_in);
//   m = B^T v, B = launch 2's map, on the hand-off words.  Launch 1 leaves, at hand-off address brev_S0(c) E2 + k,
//      Z[c][k] = omega^(c k) sum_rho x[rho E1 + c] omega^(E1 k rho)  -- the twiddle omega^(c k) rides on the butterflies of LAUNCH 1,
//      whose stages' table entries carry the row index -- in the arithmetic's lazy form, and y[kappa] = sum_c omega^(E2 j c) Z[c][k]
//      for kappa = k + E2 j.  So m[c][k] = sum_{j < E1} v[k + E2 j] (omega^(E2 c))^j: the forward column pass of v.
// Identities per vector (two-launch sizes):  sum u x == sum m z (launch 1),  sum m z as stored == as loaded (hand-off),
// sum m z == sum v y (launch 2); single-launch sizes and the whole-transform form: sum u x == sum v y.
// Not covered: faults already in the input, a fault between a tap's read of a register and the instruction that consumes the same
// register, a wrong plan handed in by the caller; a fault e at a word is invisible exactly when e * weight == 0 (mod q), which is why
// preparation refuses a plan with a zero entry in u, m or v.
// LAUNCH 0: in = u (acc_a), mid = m (acc_b; single-launch sizes: out = v); LAUNCH 1: in = m (acc_a), out = v (acc_b).
// pos0: LAUNCH 0 = the tile's first row (row0), LAUNCH 1 = address of the tile's first word inside the vector.
template <class A, int LAUNCH, int P, int S0, bool WITH_A, bool WITH_B>
struct GsTap {
    static constexpr bool ACTIVE = true;
    static constexpr bool MID = LAUNCH == 0 && WITH_B;
    static constexpr bool STORES = false;
    typedef typename A::elem elem;
    TwPtr u, m, v;                       // ArithU64: Shoup-encoded weights, from the vector's first word
    const u64 FHE_GLOBAL *u8, *m8;       // ArithF64: u and m as plain residues (v is made in registers)
    u32 pos0;
    int logp;
    elem acc_a, acc_b;
    int n_a, n_b;
    FHE_D void weigh(elem &acc, int &n, elem x, u32 at, TwPtr tw, const u64 FHE_GLOBAL *tw8, const typename A::Ctx &c)
    {
        if constexpr (A::PATH == PATH_F64) {
            const double w = A::from_canonical(tw8[at]);
            A::lazy_acc(acc, A::mulmod_w(x, w, w * c.ninv, c), ++n, c);
        } else {
            A::lazy_acc(acc, A::mulmod(x, tw[at], c), ++n, c);
        }
    }
    FHE_D void in(u32 idx, elem x, const typename A::Ctx &c)
    {
        if constexpr (WITH_A) {
            if constexpr (LAUNCH == 0) weigh(acc_a, n_a, x, (brev_bits(idx & ((1u << P) - 1u), P) << S0) + pos0 + (idx >> P), u, u8, c);
            else weigh(acc_a, n_a, x, pos0 + idx, m, m8, c);
        }
    }
    FHE_D void mid(u32 idx, elem x, const typename A::Ctx &c)
    {
        if constexpr (WITH_B) weigh(acc_b, n_b, x, (brev_bits(pos0 + (idx >> P), S0) << P) + (idx & ((1u << P) - 1u)), m, m8, c);
    }
    FHE_D void out(u32 idx, u64 y, const typename A::Ctx &c)
    {
        if constexpr (WITH_B) {
            const u32 i = LAUNCH == 0 ? idx : pos0 + idx;      // (LAUNCH 0 stores canonical words only as a single launch: one tile, row 0)
            if constexpr (A::PATH == PATH_F64) {
                const double w = ArithF64::from_canonical((u64)((i & ((1u << logp) - 1u)) + (i >> logp) + 2u));
                A::lazy_acc(acc_b, A::mulmod_w(A::from_canonical(y), w, w * c.ninv, c), ++n_b, c);
            } else {
                A::lazy_acc(acc_b, A::mulmod(A::from_canonical(y), v[i], c), ++n_b, c);
            }
        }
    }
};

// Checked product, the middle launch (k_polymul_mid_checked): for every point j of the tile, with a^_j and b^_j as the forward
// row steps leave them (the arithmetic's lazy form) and the output-side weight w^_j,
//   acc_a += w^ a^     acc_b += w^ b^     acc_ab += (w^ a^) b^
// acc_a / acc_b close the forward checks of the two factors, acc_ab is the input side of the product's check (its output side
// is sum w c over the stored result).  The sums are formed next to the product instruction, not from its result.
template <class A>
struct ProductSums {
    typedef typename A::elem elem;
    elem acc_a, acc_b, acc_ab;
    int n;
    // F64 path: w = the weight as a residue; U64 path: t = the weight in twiddle encoding
    FHE_D void add(elem a, elem b, double w, const typename A::Ctx &c)
    {
        A::reduce(a, c);                 // |.| <= q/2: the quotient estimates below stay within one unit
        A::reduce(b, c);
        const double wp = w * c.ninv;
        const elem wa = A::mulmod_w(a, w, wp, c), wb = A::mulmod_w(b, w, wp, c);
        ++n;
        A::lazy_acc(acc_a, wa, n, c);
        A::lazy_acc(acc_b, wb, n, c);
        A::lazy_acc(acc_ab, A::mulvar_lazy(wa, b, c), n, c);
    }
    FHE_D void add(elem a, elem b, const Tw &t, const typename A::Ctx &c, const LimbParams &p)
    {
        const elem wa = A::mulmod(a, t, c), wb = A::mulmod(b, t, c);     // [0, 2q) for any word
        A::lazy_acc(acc_a, wa, 0, c);
        A::lazy_acc(acc_b, wb, 0, c);
        A::lazy_acc(acc_ab, A::mulvar_lazy(wa, b, p), 0, c);              // [0, 2q) x [0, 4q): one Barrett step
    }
};

#if defined(__HIPCC__)
// modular sum of one canonical value per thread over the workgroup, stored to *dst by one lane
__device__ __forceinline__ void block_sum_mod(u64 v, u64 q, u64 *dst, u64 *red)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        v += __shfl_down(v, off, 64);
        v = v >= q ? v - q : v;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 s = 0;
        for (int w = 0; w < NTT_THREADS / 64; w++) {
            s += red[w];
            s = s >= q ? s - q : s;
        }
        *dst = s;
    }
}
#endif

} // namespace fhe
