// ntt_launch.hpp -- host-visible launch entry points of the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>

#include "fault_hook.hpp"
#include "ntt_plan.hpp"

namespace fhe {

// Batched in-place transform of a.units limbs of 2^logn points, all on `path`.
// geo: 1 = 16-column tiles (default), 0 = widest column tile (kept for 2^16 tuning runs)
// which: -1 whole transform; 0 / 1 = only the first / second launch of a two-pass size
// resident (opt-in): sizes whose limb fits a CU's LDS (2^13, 2^14) run as ONE LDS-resident pass when the whole transform is asked for
hipError_t launch_ntt(hipStream_t st, const PassArgs &a, int logn, bool inverse, int path, int geo = 1, int which = -1, bool resident = false);

// Natural-order transform (cyclic NTT of motivation/ntt.py:8-32 / the four-step flow): a.src = natural-order input,
// a.data = natural-order output (may alias), tmp = hand-off buffer of the same layout for the two-launch sizes.  The limbs'
// INVERSE table slot must hold the cyclic table (capi.cpp build_tables, GS mode).  2^5 .. 2^20.
bool ntt_gs_supported(int logn);
hipError_t launch_ntt_gs(hipStream_t st, const PassArgs &a, u64 *tmp, int logn, int path);

// Forward transform of a.data = [parts <= 3][limbs][N] whose last pass writes out_h[l] = (a_h[l] - NTT(data_h[l])) * scal[l]
// (+ add_h[l]) mod q_l instead of the transformed words (mod-down / rescale tail fused into the row pass); a_h = a + h * a_stride
// words, out / add per part, scal per limb of the run (ntt_kernels.hip k_ntt_row_subscale).  a.data is scratch afterwards.
struct RowEpiArgs {
    u64 *out[3];
    const u64 *add[3];
    const u64 *a;
    u64 a_stride;
    const u64 *scal;
    const u64 *pre = nullptr;   // optional per-limb factor applied to the transformed words first (t of the BGV forms)
    u32 galois = 0;             // != 0: the addends are sigma_k(add[h]), read through the NTT-domain Galois map (a rotation's sigma(c0))
    u32 galois_a = 0;           // != 0 (with galois): `a` is read through the same map too -- a hoisted rotation's sums, formed in the un-rotated frame
    const u64 *scal2 = nullptr; // optional second per-limb factor applied LAST: out = ((a - X) scal + add) scal2 (mod-down and rescale in one tail)
};
// Optional second input of the transform (two-launch sizes): the column pass loads data_h[l] + w[l] * y_h (mod q_l) instead of
// data_h[l]; y_h = y + h * y_stride words is ONE limb per part (residues of some other prime, any 64-bit words), w = per TABLE limb
// factors in the limb's twiddle encoding.  By linearity NTT(data + w y) = NTT(data) + w NTT(y): two subtractions share one transform.
// Round-to-nearest rescale (rescale_round.hpp): q != 0 (two-launch sizes) turns every word y < q that the column pass takes from a
// part's ONE extra limb -- the second input below, or without one the broadcast source PassArgs::src_bcast -- into the residue of
// its centred remainder, y or y - q, instead of y mod q_l; h = (q - 1) / 2.  q == 0: the flooring form, the kernels as they were
// (the host picks the column pass's rounding instantiation by q: ntt_kernels.hip k_ntt_col_addsrc<.., true>, k_ntt_col_round).
struct ColRound {
    u64 q = 0, h = 0;
};
struct ColAddSrc {
    const u64 *y;
    u64 y_stride;
    const Tw *w;
    ColRound round = {};
};
bool ntt_subscale_supported(int logn);
hipError_t launch_ntt_subscale(hipStream_t st, const PassArgs &a, const RowEpiArgs &ep, int logn, int path, const ColAddSrc *add_src = nullptr,
                               const ColRound *round = nullptr);
// the residues of a nearest rescale as words, where a launch of its own forms them (N < 2^13, test hooks, experimental transform
// variants): out[(part * limbs + l) * N + i] = centred remainder of y[part * N + i] modulo q, as a residue of q_(limb0 + l)
hipError_t launch_round_residues(hipStream_t st, u64 *out, const u64 *y, const LimbParams *lp, u32 limb0, u32 limbs, u32 n_parts, int logn, const ColRound &r);

// c = a * b mod (x^N + 1, q_l): forward column passes, one launch that finishes both forward transforms,
// multiplies and starts the inverse, inverse column pass.  a and b are scratch afterwards.
bool polymul_fused_supported(int logn);
hipError_t launch_polymul(hipStream_t st, const PassArgs &a, u64 *b, u64 *c, int logn, int path);

// forward transform with the ABFT checksums fused into the passes (ntt_kernels.hip): sum_in / sum_out are
// [units][tin] / [units][tout] partial sums (units in [poly][limb] order; tin, tout from ntt_checked_tiles);
// win / wout = [table limbs][N] weights in twiddle encoding (used by ArithU64 limbs), wout8 = output-side weights as
// residues (ArithF64 limbs; their input-side weights are computed in place).  `which` as in launch_ntt.
// inverse: the checked inverse transform -- the same tables with the sides swapped (sum_in = sum w^ X over the words the
// row pass loads, sum_out = sum w x over the words the column pass stores; abft_taps.hpp InvChecksumTap).
bool ntt_checked_supported(int logn);
void ntt_checked_tiles(int logn, u32 *tin, u32 *tout, bool inverse = false);
hipError_t launch_ntt_checked(hipStream_t st, const PassArgs &a, const Tw *win, const Tw *wout, const u64 *wout8, u64 *sum_in, u64 *sum_out,
                              int logn, int path, int which = -1, bool inverse = false);

// checked negacyclic product (launch_polymul with the detector): per limb-polynomial, in [poly][limb] order,
//   ain / bin   [units][t_in]  : sum w a, sum w b over the words the forward column passes load (one-launch sizes: the middle launch)
//   aout / bout [units][t_mid] : sum w^ a^, sum w^ b^ over the forward results as the middle launch multiplies them
//   cin         [units][t_mid] : sum w^ a^ b^, formed next to the product
//   cout        [units][t_out] : sum w c over the words the inverse column pass stores (one-launch sizes: the middle launch)
// Test hook (fault_point >= 0, one word `fault_at` and bit `fault_bit`): 0 / 1 = flip a's / b's word after its column pass,
// 2 = flip the product value at fault_at's tile position (fault_at points into a) after the multiply, 3 = flip c's word before
// the inverse column pass.
struct PolymulSums {
    u64 *ain, *bin, *aout, *bout, *cin, *cout;
    u32 t_in, t_mid, t_out;
};
struct PolymulChecks {
    const Tw *win, *wout;
    const u64 *wout8;
    PolymulSums s;
    int fault_point;
    u64 *fault_at;
    int fault_bit;
};
void polymul_checked_tiles(int logn, u32 *t_in, u32 *t_mid, u32 *t_out);
hipError_t launch_polymul_checked(hipStream_t st, const PassArgs &a, u64 *b, u64 *c, int logn, int path, const PolymulChecks &k);
// its middle launch alone (k_polymul_mid_checked with fault point 2), for a caller that runs the column passes itself
hipError_t launch_polymul_mid_checked(hipStream_t st, const PassArgs &a, u64 *b, u64 *c, int logn, int path, const PolymulChecks &k);
// flags[3 unit + k]: k = 0 / 1 / 2 = sums of a / b / the product differ (PolymulSums; tiles 1 for the unfused sequence)
hipError_t launch_compare_polymul(hipStream_t st, u32 *flags, const PolymulSums &s, const LimbParams *lp, u32 limb0, u32 limbs, u32 units);

// per-phase detector (two-launch sizes): the column pass accumulates sum w x over what it loads and sum u y over what it
// stores, the row pass sum u y over what it loads and sum w^ X over what it stores (weights: capi_abft.cpp).  One PhaseArgs
// per launch; sum_a / sum_b = that launch's [units][tiles] partial sums.  fault_*: test hook, a bit flip in the LDS image of
// workgroup fault_block of pass fault_pass between its first two phases (fault_pass < 0: off).
struct PhaseArgs {
    const Tw *win, *umid, *wout;
    const u64 *umid8, *wout8;
    int logp;
    u64 *sum_a, *sum_b;
    int fault_pass;
    u32 fault_block, fault_word;
    int fault_bit;
};
bool ntt_phases_supported(int logn);
int ntt_column_stages(int logn);   // PC of the size's plan (0 for single-launch sizes)
hipError_t launch_ntt_phases(hipStream_t st, const PassArgs &a, const PhaseArgs &p1, const PhaseArgs &p2, int logn, int path, int which = -1);
// flags[unit*3 + {0,1,2}] = column pass / hand-off / row pass checks failed; s_in, s_mid1 have `tc` partial sums per unit,
// s_mid2, s_out `tr`
hipError_t launch_compare_phases(hipStream_t st, u32 *flags, const u64 *s_in, const u64 *s_mid1, u32 tc, const u64 *s_mid2, const u64 *s_out, u32 tr,
                                 const LimbParams *lp, u32 limb0, u32 limbs, u32 units);

// ---- fourstep_checked.hip: launch_ntt_gs with the detector (abft_taps.hpp GsTap), one modulus (a.limbs == 1, unit = vector) ----
// One GsCheckArgs per launch.  u / m / v = [N] weights in twiddle encoding (integer path), u8 / m8 = u and m as residues (FP64 path,
// which makes v in registers); m may be null for single-launch sizes.  sum_a / sum_b = that launch's [vectors][tiles] partial sums
// (tiles from ntt_gs_checked_tiles): launch 1 sum u x / sum m z (single-launch sizes: sum v y), launch 2 sum m z / sum v y.
// phases = false (whole-transform form): launch 1 fills only sum_a, launch 2 only sum_b.  fault_*: test hook of the per-phase form,
// a bit flip in the LDS image of workgroup fault_block of launch fault_pass between its first two register steps (< 0: off).
// which as in launch_ntt (the between-launch hook splits the launches).
struct GsCheckArgs {
    const Tw *u, *m, *v;
    const u64 *u8, *m8;
    int logp;
    u64 *sum_a, *sum_b;
    int fault_pass;
    u32 fault_block, fault_word;
    int fault_bit;
};
void ntt_gs_checked_tiles(int logn, u32 *t1, u32 *t2);
hipError_t launch_ntt_gs_checked(hipStream_t st, const PassArgs &a, u64 *tmp, const GsCheckArgs &c1, const GsCheckArgs &c2, int logn, int path,
                                 bool phases, int which = -1);

// packed hand-off between the two launches (forward 2^16, FP64 limbs): when PassArgs::scratch is set (ntt_packed_scratch_words()
// 64-bit words per unit) the intermediate travels as 50-bit residues in 16x16 blocks instead of 8-byte words in place
bool ntt_packed_supported(int logn, bool inverse, int path);
size_t ntt_packed_scratch_words();

// ---- ntt_fused.hip: single-launch variant for two-pass sizes --------------------
bool fused_supported(int logn);
size_t fused_ctl_bytes(u32 units);
// variant = handoff * 2 + stream_hint, handoff: 1 sc1 loads, 2 nt loads, 3 acquire + plain loads
hipError_t launch_ntt_fused(hipStream_t st, const PassArgs &a, int logn, bool inverse, int path, u32 *ctl, u32 dist, u32 wgs,
                            int variant, u32 skip_teams);

// ---- aux_kernels.hip --------------------------------------------------------
struct PointwiseArgs {
    u64 *c;
    const u64 *a;
    const u64 *b;
    const LimbParams *lp;
    u32 limb0, limbs, units, poly_stride;
    int logn;
};
// c = a*b mod q (accumulate = false) or c = (c + a*b) mod q (accumulate = true), per limb
hipError_t launch_modmul(hipStream_t st, const PointwiseArgs &p, bool accumulate);
// tensor product of two two-part ciphertexts, NTT domain, per limb: d0 = a0 b0, d1 = a0 b1 + a1 b0, d2 = a1 b1
// (the coefficient-wise core of phantom::multiply, reliability_test/dotprod_test.cu:113); every operand [limbs][N]
struct TensorArgs {
    u64 *d0, *d1, *d2;
    const u64 *a0, *a1, *b0, *b1;
    const LimbParams *lp;
    u32 limb0, limbs;
    int logn;
};
hipError_t launch_tensor(hipStream_t st, const TensorArgs &p);
// ---- pointwise_checked.hip: the same products with a residue check per word (residue_check.hpp) --------
// flags: one uint32 per limb-polynomial (modmul) or [limb][3] (tensor), zeroed by the caller; a word that fails ORs in
// its flag bits.  The check record BcCheck: fault_hook.hpp; its unit is the limb-polynomial poly * limbs + l (modmul) or the
// limb, where the fault hits the d1 sum (tensor product)
hipError_t launch_modmul_checked(hipStream_t st, const PointwiseArgs &p, bool accumulate, const BcCheck &k);
hipError_t launch_tensor_checked(hipStream_t st, const TensorArgs &p, const BcCheck &k);
// inner sum of a BSGS matrix-vector product: out_h = sum_b diag[b] * R_b,h per limb (aux_kernels.hip k_diag_mac); diag = [n1][limbs][N],
// R_0 = (x0, x1), R_b = rot + (b - 1) * 2 * limbs * N ([n1 - 1][2][limbs][N])
struct DiagMacArgs {
    u64 *out0, *out1;
    const u64 *diag, *x0, *x1, *rot;
    const LimbParams *lp;
    u32 limb0, limbs, n1;
    int logn;
};
// term b at word e = (l << logn) + i as the checked and the sealed inner sum load it, each operand as a V (one word, or two adjacent
// ones): d = the diagonal, y0 / y1 = the two parts of R_b
template <class V> FHE_HD void diag_mac_load(const DiagMacArgs &a, u32 b, u64 e, V &d, V &y0, V &y1)
{
    const u64 part = (u64)a.limbs << a.logn;
    d = *reinterpret_cast<const V *>(a.diag + ((u64)b * part + e));
    const u64 *r = b ? a.rot + (u64)(b - 1) * 2 * part : nullptr;
    y0 = b ? *reinterpret_cast<const V *>(r + e) : *reinterpret_cast<const V *>(a.x0 + e);
    y1 = b ? *reinterpret_cast<const V *>(r + (part + e)) : *reinterpret_cast<const V *>(a.x1 + e);
}
hipError_t launch_diag_mac(hipStream_t st, const DiagMacArgs &a);
hipError_t launch_modadd(hipStream_t st, const PointwiseArgs &p);
hipError_t launch_modsub(hipStream_t st, const PointwiseArgs &p);
constexpr int SCALAR_MAX_LIMBS = 64;
struct ScalarVec {
    u64 v[SCALAR_MAX_LIMBS];
};
// c = a * mul[l] + add[l] mod q_l (per-limb scalars, reduced by the caller)
hipError_t launch_scalar_affine(hipStream_t st, const PointwiseArgs &p, const ScalarVec &mul, const ScalarVec &add);
// data[idx] ^= 1 << bit  (reliability_test/dotprod_test.cu:31-33)
hipError_t launch_flip_bit(hipStream_t st, u64 *data, u64 idx, int bit);
// modulus + floor(2^128/q) for the Barrett helpers, passed by value
struct ModConst {
    u64 q, r0, r1;
};
// per unit of 2^logn words: dst[i] = src[bitrev(i)] (* scale mod q when do_scale).  dst != src.
hipError_t launch_bitrev_scale(hipStream_t st, u64 *dst, const u64 *src, int logn, u32 units, const ModConst &mc, u64 scale,
                               bool do_scale);
// per vector of rows x cols words: dst[c][r] = src[r][c] (* w^(r c) mod q when tlo != nullptr, w^e = tlo[e mod 2^lo_bits] * thi[e >> lo_bits])
hipError_t launch_transpose_tw(hipStream_t st, u64 *dst, const u64 *src, u32 rows, u32 cols, u32 n_vec, const ModConst &mc, const u64 *tlo, const u64 *thi,
                               int lo_bits);
// out_h = (a_h - b_h) * scal[l] (+ add_h) mod q_l over `limbs` limbs from table index limb0, for one half
// (out1 == nullptr) or both halves of a key switch in one launch; a_h = a + h * a_stride, b_h = b + h * b_stride (in words);
// a == nullptr / b == nullptr: that operand is zero
struct SubScaleArgs {
    u64 *out0, *out1;
    const u64 *a, *b, *add0, *scal;
    u64 a_stride, b_stride;
    const LimbParams *lp;
    u32 limb0, limbs;
    int logn;
    const u64 *add1 = nullptr;
};
hipError_t launch_sub_scale(hipStream_t st, const SubScaleArgs &p);
// out[unit] = sum_i w[limb][i] * x[unit][i] mod q_limb (one workgroup per limb-polynomial): the weighted
// checksum of the reference's ECC (rfhe_framewk/src/negaclic_ntt.py:130-149); scal[limb] multiplies the sum
hipError_t launch_weighted_checksum(hipStream_t st, u64 *out, const u64 *x, const u64 *w, const u64 *scal, const LimbParams *lp,
                                    u32 limb0, u32 limbs, u32 units, u32 poly_stride, int logn);
// out[unit] = scal[limb] * sum_i w[limb][i] * x[unit][i] * y[unit][i] mod q_limb: the input side of the unfused product's check
hipError_t launch_weighted_checksum3(hipStream_t st, u64 *out, const u64 *x, const u64 *y, const u64 *w, const u64 *scal, const LimbParams *lp,
                                     u32 limb0, u32 limbs, u32 units, u32 poly_stride, int logn);
// flags[unit] = a[unit] != b[unit]
hipError_t launch_compare_flags(hipStream_t st, u32 *flags, const u64 *a, const u64 *b, u32 units);
// flags[unit] = (sum of a[unit][0..ta) mod q_l) != (sum of b[unit][0..tb) mod q_l)  (unit = poly * limbs + l)
hipError_t launch_compare_sums(hipStream_t st, u32 *flags, const u64 *a, u32 ta, const u64 *b, u32 tb, const LimbParams *lp, u32 limb0,
                               u32 limbs, u32 units);
// Galois automorphism x -> x^k: coefficient domain (sign-aware scatter) and NTT domain (gather)
hipError_t launch_automorphism(hipStream_t st, u64 *dst, const u64 *src, const LimbParams *lp, u32 limb0, u32 limbs, u32 units,
                               int logn, u32 k);
// optional second (destination, source) pair of the same shape in the same launch
hipError_t launch_automorphism_ntt(hipStream_t st, u64 *dst, const u64 *src, u32 units, int logn, u32 k, u64 *dst_b = nullptr,
                                   const u64 *src_b = nullptr);

// ---- baseconv_kernels.hip ------------------------------------------------------
struct BaseConvPlanDev {
    int m, k;
    const u64 *mod_in;        // m
    const u64 *mod_out;       // k
    // exact conversion, mixed-radix digits c_j = r_j*A_j - sum_{l<j} c_l*D_lj (mod p_j) and x = sum_l c_l*E_lo (mod q_o):
    const Tw *dig;            // m x m   [j*m+j] = A_j = (p_0..p_{j-1})^-1 mod p_j;  [l*m+j], l<j = D_lj = (p_l..p_{j-1})^-1 mod p_j
    const Tw *hor;            // m x k   E_lo = p_0..p_{l-1} mod q_o
    const Tw *fp_in, *fp_out; // m, k    {bits((double)q), bits(1.0/q)} per modulus (ArithF64 context)
    int f64;                  // 1: every modulus < 2^50, constants encoded for ArithF64; 0: Shoup pairs (ArithU64)
    const u64 *fast_coef;     // m x k   (Phat_j * inv_j) mod q_o   (rfhe_framewk/src/baseConv.py:17-29)
    const u64 *fast_coef_shoup;
    // m <= 16: the same constants laid out as the fixed-size kernels keep them in LDS, so that a workgroup stages them with ONE batch
    // of 16-byte loads: img_head = dig [m][m], fp_in [m], mod_in [m] (two per entry); img_out = per output o: hor[0..m-1][o], fp_out[o],
    // {mod_out[o], 0} -- m + 2 entries per output, a slice of outputs is a contiguous range
    const Tw *img_head;
    const Tw *img_out;
    const u32 *rows_identity; // 0, 1, 2, ... (64 entries): the row map of a job that has none
};
// output limb o is written at limb index o (o < gap_at) or o + gap: lets a key-switch digit's extension land
// in the [M][N] layout with the digit's own limbs skipped
struct BcJob;
hipError_t launch_baseconv_exact(hipStream_t st, u64 *out, const u64 *in, const BaseConvPlanDev &pl, u64 N, u32 gap_at = 0xFFFFFFFFu,
                                 u32 gap = 0, const u32 *in_rows = nullptr);
struct BcJob {
    BaseConvPlanDev pl;
    const u64 *in;
    u64 *out;
    u32 gap_at, gap;
    const u32 *in_rows = nullptr;   // optional: input limb j sits at row in_rows[j] of `in` (rows of N words) instead of row j --
                                    // the all-gathered slabs of a sharded key switch are padded per rank
};
// m_mask: bit (m - 1) set for every input size m <= 16 among the jobs (one straight-line launch per size); 0 = the runtime-m kernels
hipError_t launch_baseconv_exact_jobs(hipStream_t st, const BcJob *dev_jobs, u32 n_jobs, int max_m, int max_k, bool f64, u64 N, u32 m_mask = 0);
// key-switch inner product over all digits and both key halves (aux_kernels.hip k_ks_mac).  Rows are the limbs this
// rank owns: cn ciphertext limbs (table limbs clo ..) followed by the owned special limbs (table limb = row + sp_shift);
// one device owns everything: M = L + K, cn = L, clo = 0, sp_shift = 0.
struct KsMacArgs {
    u64 *acc;            // [2][M][N]
    const u64 *ext;      // [dnum][M][N]  extended digits, NTT form (the digit's own limbs unused)
    const u64 *c;        // [cn][N]       owned input limbs, NTT form
    const u64 *evk;      // [dnum][2][M][N]
    const LimbParams *lp;
    u32 L, M, dnum, alpha;
    int logn;
    u32 cn, clo, sp_shift;
};
// the table limb of row j when it is a ciphertext limb (no limb otherwise): a row's own invariant, hoisted by the caller
FHE_HD u32 ks_mac_table_limb(const KsMacArgs &a, u32 j) { return j < a.cn ? a.clo + j : 0xFFFFFFFFu; }
// term d at word i of row j (table limb tl) as the checked and the sealed inner product load it: x = the digit as a V (one word, or
// two adjacent ones) -- from the owned limb of c where the row is a ciphertext limb of the digit's own range, from the digit's
// extension elsewhere -- and the address of half 0 of the key (half 1: M N words on), which each kernel loads in its own way
template <class V> FHE_HD const u64 *ks_mac_load(const KsMacArgs &a, u32 tl, u32 d, u32 j, u64 i, V &x)
{
    const u64 N = (u64)1 << a.logn;
    const u32 lo = d * a.alpha, hi = lo + a.alpha < a.L ? lo + a.alpha : a.L;
    x = (tl >= lo && tl < hi) ? *reinterpret_cast<const V *>(a.c + ((u64)j * N + i)) : *reinterpret_cast<const V *>(a.ext + (((u64)d * a.M + j) * N + i));
    return a.evk + ((u64)d * 2 * a.M + j) * N + i;
}
hipError_t launch_ks_mac(hipStream_t st, const KsMacArgs &a);
// n <= 4 keys on the same digits: acc[r] = sum_d ext_d * evk[r][d] (a.acc / a.evk unused)
struct KsMacMultiArgs {
    KsMacArgs a;
    u32 n;
    const u64 *evk[4];
    u64 *acc[4];
};
hipError_t launch_ks_mac_multi(hipStream_t st, const KsMacMultiArgs &m);
// The same inner product with the LAST pass of the extended limbs' forward transform fused in (ntt_kernels.hip k_ks_rowmac):
// `ext` then holds what the transform's first launch left (the column pass's lazy words; for single-pass sizes the
// base-extension output itself), one workgroup per (owned limb, row tile) runs the row pass of every digit's limb in LDS,
// multiplies by the two key halves and keeps the sums in registers: the transformed digits are never written or re-read.
bool ks_rowmac_supported(int logn);
hipError_t launch_ks_rowmac(hipStream_t st, const KsMacArgs &a, bool has_f64, bool has_u64);
hipError_t launch_bconv_fast(hipStream_t st, u64 *out, const u64 *in, const BaseConvPlanDev &pl, u64 N);
hipError_t launch_crt_garner(hipStream_t st, u64 *x_lo, u64 *x_hi, const u64 *residues, const u64 *moduli,
                             const u64 *ratios, const u64 *pref_lo, const u64 *pref_hi, const u64 *inv_pref, int m, u64 N);
hipError_t launch_bsgs_hadamard(hipStream_t st, u64 *y, const u64 *M_blocks, const u64 *v, int k, int bs,
                                const ModConst *mc /* nullptr: int64 wrap-around like the reference */);

// ---- baseconv_checked.hip: the two conversions with a residue check per digit and per output word (baseconv_check.hpp) ----
// flags: exact [m + k] (digit units, then output units), fast [k]; the check record BcCheck: fault_hook.hpp
// a conversion as the unchecked launcher describes it (BcJob: output gap, input row map) plus what the check needs: the digit and
// output tables as Shoup pairs {w, floor(w 2^64 / q)} in the layout of BaseConvPlanDev::dig / hor -- the plan's own tables on
// integer plans, a second pair of tables on FP64 plans
struct BcCheckedJob {
    BcJob job;
    const Tw *dig, *hor;
    BcCheck chk;
};
hipError_t launch_baseconv_exact_checked(hipStream_t st, const BcCheckedJob &cj, u64 N);
hipError_t launch_bconv_fast_checked(hipStream_t st, u64 *out, const u64 *in, const BaseConvPlanDev &pl, const BcCheck &chk, u64 N);

// ---- keyswitch_checked.hip: the key switch's inner product and mod-down tail with a residue check per word (keyswitch_check.hpp) ----
// launch_ks_mac / launch_sub_scale with a check record: flags [2][M] (half, row) / [halves][limbs], zeroed by the caller;
// fault_point >= 0: XOR fault_mask at that injection point of unit fault_unit (index into flags), coefficient fault_coeff
hipError_t launch_ks_mac_checked(hipStream_t st, const KsMacArgs &a, const BcCheck &k);
hipError_t launch_sub_scale_checked(hipStream_t st, const SubScaleArgs &p, const BcCheck &k);
// dst[map[i]] = src[i] for the non-zero src[i], i < n
hipError_t launch_ks_flags_scatter(hipStream_t st, u32 *dst, const u32 *src, const u32 *map, u32 n);

// ---- rescale_checked.hip: the residues of a rescale's dropped limb with a residue check per word (rescale_check.hpp) ----
// delta[part][j][i] = x[part][i] mod q_j for the table limbs j < R, x = [n_parts][N] words below q_R (the dropped limb in
// coefficient form); flags [n_parts][R], zeroed by the caller; the check record as for launch_ks_mac_checked
struct RescaleReduceArgs {
    u64 *delta;          // [n_parts][R][N]
    const u64 *x;        // [n_parts][N]
    const LimbParams *lp;
    u32 R, n_parts;
    int logn;
};
hipError_t launch_rescale_reduce_checked(hipStream_t st, const RescaleReduceArgs &a, const BcCheck &k);

// ---- galois_checked.hip: the NTT-domain Galois permutation with a position-weighted sum check per unit (galois_check.hpp) ----
// launch_automorphism_ntt's words; adds the unit's source-side and destination-side sums into s_in / s_out ([units] each, zeroed by
// the caller), kinv = k^-1 mod 2N; f.point >= 0: the one-shot test fault.  launch_galois_compare: flags[unit] = the sums differ
// modulo 2^32 - 1 (every unit's word is written)
struct GaloisFault;
hipError_t launch_automorphism_ntt_checked(hipStream_t st, u64 *dst, const u64 *src, u64 *s_in, u64 *s_out, u32 units, int logn, u32 k, u32 kinv,
                                           const GaloisFault &f);
hipError_t launch_galois_compare(hipStream_t st, u32 *flags, const u64 *s_in, const u64 *s_out, u32 units);

// ---- bsgs_checked.hip: the inner sum of the BSGS product and the modular add with a residue check per word (bsgs_check.hpp) ----
// launch_diag_mac / launch_modadd with a check record: flags [2][limbs] (part, limb) / [units] (poly * limbs + l), zeroed by the
// caller; fault_point >= 0: XOR fault_mask at that injection point of unit fault_unit (index into flags), coefficient fault_coeff
hipError_t launch_diag_mac_checked(hipStream_t st, const DiagMacArgs &a, const BcCheck &k);
hipError_t launch_modadd_checked(hipStream_t st, const PointwiseArgs &p, const BcCheck &k);

// ---- scalar_checked.hip: the scalar multiply / affine map with a residue check per word (scalar_check.hpp) ----
// launch_scalar_affine with a check record (p.b unused; add == nullptr: no addend, and no injection point 3): flags [units]
// (poly * limbs + l), zeroed by the caller; fault_point >= 0: XOR fault_mask at that injection point of unit fault_unit (index
// into flags), coefficient fault_coeff
hipError_t launch_scalar_affine_checked(hipStream_t st, const PointwiseArgs &p, const ScalarVec &mul, const ScalarVec *add, const BcCheck &k);

// ---- seal_checked.hip: seals of rows at rest, two weighted sums modulo 2^61 - 1 per row (seal_check.hpp) ----
// the rows of a window of limbs of n_poly polynomials poly_stride rows apart, addressed as PointwiseArgs addresses them; x is
// 16-byte aligned and logn >= 1 (a lane loads two words)
struct SealArgs {
    const u64 *x;
    const LimbParams *lp;
    u32 limb0, limbs, units, poly_stride;
    int logn;
};
// words of the partial-sum scratch a launch needs: [units][chunks per row][2]
size_t seal_part_words(u32 units, int logn);
// seal[unit] = {S0, S1}, canonical; fault_point >= 0: XOR fault_mask into word fault_coeff of row fault_unit in the register
hipError_t launch_seal(hipStream_t st, const SealArgs &p, u64 *part, u64 *seal, const BcCheck &k);
// k.flags[unit] |= SEAL_SUM where the row's sums differ from seal[unit], SEAL_RANGE where a word is >= q_l; zeroed by the caller
hipError_t launch_seal_verify(hipStream_t st, const SealArgs &p, u64 *part, const u64 *seal, const BcCheck &k);

// ---- seal_repair.hip: the locator sum S2 per row and the repair of one corrupted word per row (seal_check.hpp) ----
// locator[unit] = S2, canonical; part as launch_seal's (half of it is used)
hipError_t launch_seal_locator(hipStream_t st, const SealArgs &p, u64 *part, u64 *locator);
// after launch_seal_verify filled flags: every row with a raised flag is re-read, decided (seal_decide) and, where exactly one word
// is named, corrected in place and confirmed; flags[unit] = 0 after a confirmed repair or a clean re-read, untouched otherwise;
// report[unit] = {status, index, word before, word after}.  p.x is written: the caller owns it as mutable memory
hipError_t launch_seal_repair(hipStream_t st, const SealArgs &p, const u64 *seal, const u64 *locator, u32 *flags, u64 *report);

// ---- seal_carry.hip: the modular add / subtract that carries its operands' seals to the result (seal_carry.hpp) ----
// words of the partial-sum scratch a launch needs: [units][chunks per row][4, or 6 with locators]
size_t carry_part_words(u32 units, int logn, bool loc);
// launch_modadd's / launch_modsub's words (p.a, p.b, p.c 16-byte aligned, logn >= 1; c may be a or b); seal_c[unit] = the sums
// predicted from seal_a, seal_b and the wraps, and loc_c[unit] from loc_a, loc_b when loc_c != nullptr; k.flags[unit] |= SEAL_SUM
// where the digest of c as stored differs from the prediction, SEAL_RANGE where an operand word is >= q_l; zeroed by the caller.
// k.fault_point >= 0: the test fault at that point (CARRY_AT_*) of word fault_coeff of row fault_unit, in the register
hipError_t launch_modadd_carry(hipStream_t st, const PointwiseArgs &p, bool sub, u64 *part, const u64 *seal_a, const u64 *seal_b, u64 *seal_c,
                               const u64 *loc_a, const u64 *loc_b, u64 *loc_c, const BcCheck &k);

// ---- mac_sealed.hip: the inner sum of the BSGS product with the diagonals' seals verified on the consuming load (mac_seal.hpp) ----
// the compile-time bound on the baby steps the launch picks for n1 <= DIAG_SEAL_MAX_NB: the smallest of 4, 8, 16 that holds n1
u32 diag_seal_nb(u32 n1);
// words of the partial-sum scratch a launch needs: room for [limbs][chunks per row][nb][2], of which a job writes [n1][2]
size_t diag_seal_part_words(u32 limbs, int logn, u32 nb);
// launch_diag_mac_checked's words and flags (k) with every buffer of a 16-byte aligned, logn >= 1 and n1 <= DIAG_SEAL_MAX_NB;
// seal = [n1 * limbs][2] the stored seals of this giant step's diagonal rows (row b * limbs + l); seal_flags[b * limbs + l] |=
// SEAL_SUM where the row as loaded differs from its seal, SEAL_RANGE where a word is >= q_l; zeroed by the caller.  hit.mask != 0:
// the sealed call's test fault, in the register as loaded (bsgs_seal.hpp)
struct DiagHit;
hipError_t launch_diag_mac_sealed(hipStream_t st, const DiagMacArgs &a, u64 *part, const u64 *seal, u32 *seal_flags, const BcCheck &k, const DiagHit &hit);

// ---- tensor_sealed.hip: the tensor product with its operands' seals verified on the multiplying load (tensor_seal.hpp) ----
// launch_tensor_checked's words over rows [units] = [n_poly][limbs] (row u on table limb limb0 + u % limbs, at word u << logn of
// every buffer), every buffer 16-byte aligned, logn >= 1.  seal_in[o] = [units][2] the stored seal of operand o (a0, a1, b0, b1) or
// null: not compared; flags_op[o][u] |= SEAL_SUM where the row as loaded differs from it, SEAL_RANGE where a word is >= q_l (always
// checked).  seal_out[i] = [units][2] receives the digest of d_i as stored, or null; all null: nothing is digested
struct TensorSealArgs {
    u64 *d0, *d1, *d2;
    const u64 *a0, *a1, *b0, *b1;
    const LimbParams *lp;
    u32 limb0, limbs, units;
    int logn;
    const u64 *seal_in[4];
    u64 *seal_out[3];
    u32 *flags_op[4];
};
// the sealed call's test fault as a launch reads it: XOR mask into word coeff of row `row` of operand op, in the register as loaded
// (mask == 0: not armed)
struct TensorSealHit {
    int op;
    u32 row;
    u64 coeff, mask;
};
// every sealed launcher's cap on the workgroups of its job loop (seal_sweep.hpp)
constexpr u32 TENSOR_SEAL_GRID_CAP = 8192;
// words of the partial-sum scratch a launch needs: [units][chunks per row][8, or 14 with output seals]
size_t tensor_seal_part_words(u32 units, int logn, bool out);
// k.flags = [units][3] the residue flags of d0, d1, d2 (zeroed by the caller, as flags_op); k's fault: the d1 sum of word fault_coeff
// of row fault_unit
hipError_t launch_tensor_sealed(hipStream_t st, const TensorSealArgs &t, u64 *part, const BcCheck &k, const TensorSealHit &hit);

// ---- mac_sealed.hip: the key switch's inner product with the key's seal verified on the multiplying load (mac_seal.hpp) ----
// the sealed call's test fault as a launch reads it: XOR mask into word coeff of key row key_row = (d 2 + h) M + j, in the register
// as loaded (mask == 0: not armed)
struct KsSealHit {
    u32 key_row;
    u64 coeff, mask;
};
// the compile-time bound on the digits the launch picks for dnum <= KS_SEAL_MAX_DNUM: the smallest of 2, 4, 8, 12 that holds dnum
u32 ks_seal_nd(u32 dnum);
// words of the partial-sum scratch a launch needs: [M][chunks per row][2 dnum][2] -- what a sweep over the key's rows needs
size_t ks_seal_part_words(u32 M, int logn, u32 dnum);
// launch_ks_mac_checked's words and flags (k) with a.c, a.ext, a.evk and a.acc 16-byte aligned, logn >= 1 and dnum <=
// KS_SEAL_MAX_DNUM; seal_key = [dnum 2 M][2] the stored seals of the key's rows or null: not compared; flags_key[(d 2 + h) M + j] |=
// SEAL_SUM where the row as loaded differs from its seal, SEAL_RANGE where a word is >= q_j (always checked); zeroed by the caller
hipError_t launch_ks_mac_sealed(hipStream_t st, const KsMacArgs &a, u64 *part, const u64 *seal_key, u32 *flags_key, const BcCheck &k, const KsSealHit &hit);

// ---- galois_sealed.hip: the Galois permutation with the source's seal verified and the destination's written on its one gather (galois_seal.hpp) ----
// rows addressed as SealArgs addresses them; dst and src 16-byte aligned and distinct, logn >= 1 (a lane stores two words), k odd
struct GalSealArgs {
    u64 *dst;
    const u64 *src;
    const LimbParams *lp;
    u32 limb0, limbs, units, poly_stride;
    int logn;
    u32 k;
};
// the sealed permutation's test fault as a launch reads it: point < 0 = not armed; mask = the bit, of the gathered word (GAL_AT_WORD)
// or of the source index (GAL_AT_INDEX, below 2^logn), at destination word coeff of row `row`
struct GalSealHit {
    int point;
    u32 row, coeff;
    u64 mask;
};
// words of the partial-sum scratch a launch needs: [units][chunks per row][3, or 4 with a destination seal]
size_t galois_seal_part_words(u32 units, int logn, bool out);
// launch_automorphism_ntt's words; flags[unit] |= SEAL_SUM where the row as gathered differs from seal_src[unit] ([units][2],
// required), SEAL_RANGE where a word is >= q_l; zeroed by the caller.  seal_dst != nullptr: seal_dst[unit] = {seal_src[unit][0] as
// stored, the digested S1 of the destination} (may be seal_src)
hipError_t launch_automorphism_ntt_sealed(hipStream_t st, const GalSealArgs &a, u64 *part, const u64 *seal_src, u64 *seal_dst, u32 *flags,
                                          const GalSealHit &hit);

// ---- ntt_sealed.hip, ntt_fwd_sealed.hip: the checked transforms with their input's seal verified on the transform's own load and
// their output sealed on store (ntt_seal_tap.hpp, ntt_sealed_io.hpp) ----
// what the sealed first launch needs beside launch_ntt_checked's arguments.  Rows are addressed as the detector's sums are: row
// (poly, l) of the launch at index poly * a.poly_stride + l of seal_src ([rows][2], or null: not compared), flags ([rows]: every
// row's word is WRITTEN -- SEAL_SUM where the row as the transform loaded it differs from its seal, SEAL_RANGE where a word is
// >= q_l) and part (ntt_seal_part_words(rows, logn, inverse) words).  hit_mask != 0: the test fault, XOR into word hit_coeff of row
// hit_row in the register as loaded
struct NttSealIn {
    const u64 *seal_src;
    u32 *flags;
    u64 *part;
    u32 hit_row = 0, hit_coeff = 0;
    u64 hit_mask = 0;
};
// words of the input digest's partials, [rows][tiles of the loading launch][3], and of the output digest's, [rows][tiles of the
// storing launch][2].  The two regions are distinct: the single pass writes both in one launch
size_t ntt_seal_part_words(u32 rows, int logn, bool inverse);
size_t ntt_seal_out_part_words(u32 rows, int logn, bool inverse);
// launch_ntt_checked with the first launch (forward: the column pass, inverse: the row pass; below 2^13 the single pass) sealed as
// NttSealIn describes, and the storing launch digesting every word it stores into part_out, addressed as s.part is.  part_out ==
// nullptr: no output seal (two-launch sizes: the second launch is launch_ntt_checked's own).  `which` as there (0: the sealed first
// launch and its verdict, 1: the second launch), so the between-launch flip hook of the checked stages keeps working.  a.src
// (optional, mirrored layout): the first launch reads the sealed rows from there and a.data receives the result -- out of place, no
// copy.  Whole-batch launches only: a.map, a.tmp, a.scratch, a.src_bcast, a.src_stride, a.stream_hint and a.galois must be unset.
// ntt_checked_supported sizes
hipError_t launch_ntt_sealed(hipStream_t st, const PassArgs &a, const Tw *win, const Tw *wout, const u64 *wout8, u64 *sum_in, u64 *sum_out, int logn, int path,
                             int which, bool inverse, const NttSealIn &s, u64 *part_out);
// k_ntt_seal_finish over the rows of launch `a`, whose first launch left `tiles` partials per row at s.part
hipError_t launch_ntt_seal_finish(hipStream_t st, const PassArgs &a, u32 tiles, const NttSealIn &s);
// one lane per row: seal_dst[row] = the row's merged output digest, canonical, where flags_in[row] and flags_abft[row] are both
// zero, {~0, ~0} otherwise (ntt_seal_out).  Runs after the verdicts and launch_compare_sums on the same stream.  flags_in2 (optional):
// a second verdict block, [rows], counted with the first; abft_words: the ABFT block holds that many words per row, any of them
// raised poisons the row (the sealed product: two factors' verdicts and launch_compare_polymul's three words)
hipError_t launch_ntt_seal_out_finish(hipStream_t st, const u64 *part_out, u32 tiles, u32 rows, const u32 *flags_in, const u32 *flags_abft, u64 *seal_dst,
                                      const u32 *flags_in2 = nullptr, u32 abft_words = 1);

// ---- polymul_sealed.hip: launch_polymul_checked with both factors' seals verified on the loads that transform them and the product
// sealed from the words the last launch stores (polymul_seal.hpp) ----
// Rows are addressed as the detector's sums are (NttSealIn).  a / b: the factors' records -- seal, flag block and partials
// ([rows][t_in][3] each, t_in from polymul_checked_tiles); b is not read when squaring (b == a.data): the caller copies a's verdicts.
// part_c: [rows][t_out][2] partials of the product's digest, or null: no output seal.  The test fault of either record (hit_mask
// != 0) is applied in the register as the loading launch takes the word; squaring applies a's to both loads of the single launch.
// Whole-batch launches only (launch_ntt_sealed's conditions on the PassArgs)
struct PolymulSealIo {
    NttSealIn a, b;
    u64 *part_c;
};
hipError_t launch_polymul_sealed(hipStream_t st, const PassArgs &a, u64 *b, u64 *c, int logn, int path, const PolymulChecks &k, const PolymulSealIo &io);

// ---- subscale_sealed.hip: the mod-down tail with its first operand verified on load and its result sealed on store (subscale_seal.hpp) ----
// what the sealed tail needs beside launch_sub_scale_checked's arguments.  Rows are (half h, limb l) of the launch.  seal_out0 /
// seal_out1 = [limbs][2] receive the seal of out0 / out1 from the registers that are stored (either may be null: that half is not
// sealed).  flags_in != nullptr selects the IN form: row (h, l) of p.a is digested on the load that subtracts from it and held
// against seal_in[h * in_stride + l] ([..][2], or null: not compared); flags_in[h * in_stride + l] |= SEAL_SUM where they differ,
// SEAL_RANGE where a word is >= q_l; zeroed by the caller.  hit_point >= 0: the sealed tail's test fault (SS_AT_LOAD needs the IN
// form), XOR hit_mask into word hit_coeff of row hit_row = h * limbs + l
struct SubScaleSeal {
    u64 *part;      // subscale_seal_part_words(rows, logn, IN) words
    u64 *seal_out0, *seal_out1;
    const u64 *seal_in = nullptr;
    u32 *flags_in = nullptr;
    u32 in_stride = 0;
    int hit_point = -1;
    u32 hit_row = 0, hit_coeff = 0;
    u64 hit_mask = 0;
};
// words of the partial-sum scratch a launch needs: [rows][chunks per row][2, or 4 in the IN form]
size_t subscale_seal_part_words(u32 rows, int logn, bool in);
// launch_sub_scale_checked's words and flags (k) with every buffer of p 16-byte aligned and logn >= 1
hipError_t launch_sub_scale_sealed(hipStream_t st, const SubScaleArgs &p, const BcCheck &k, const SubScaleSeal &s);

} // namespace fhe
