/*
 * fhe_mi355x.h -- C ABI of libfhe_mi355x.so, the MI355X (gfx950) negacyclic-NTT /
 * RNS polynomial-arithmetic engine.
 *
 * Plain C: opaque handles, raw device addresses, sizes; every function returns an
 * int status (0 = FHE_OK) and never throws across the boundary; fhe_last_error()
 * gives the text of the last failure on the calling thread.  All work is enqueued
 * on the stream passed in (a hipStream_t as void*; NULL = the context's own
 * stream); the caller synchronises (fhe_sync), exactly as the reference's harness
 * does around the Phantom calls (reliability_test/ntt_test.cu:88-102).
 *
 * Each entry point cites the reference interface it stands in for.  Paths are
 * relative to the Stardust-lf/fhe-reliability-gpu tree.  "Phantom" symbols are the
 * ones the reference's binaries import from the (absent) libPhantom.so
 * (nm -D reliability_test/build/ntt_test).
 *
 * Data layout: residue polynomials are limb-major, [n_poly][limbs][N] uint64_t,
 * contiguous (h_data[i*dim + j], reliability_test/ntt_test.cu:79).
 * Semantics: every 64-bit input word is first taken modulo its limb's modulus, all
 * outputs are canonical residues in [0, q).
 */
#ifndef FHE_MI355X_H
#define FHE_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FHE_OK 0
#define FHE_ERR_INVALID 1     /* bad argument */
#define FHE_ERR_HIP 2         /* HIP runtime error, see fhe_last_error() */
#define FHE_ERR_UNSUPPORTED 3 /* size / modulus outside what the kernels handle */
#define FHE_ERR_NOMEM 4

#define FHE_PATH_F64 0 /* q < 2^50: exact FP64 arithmetic (reference prime size, ntt_test.cu:44) */
#define FHE_PATH_U64 1 /* q < 2^61: 64-bit Shoup / Harvey arithmetic */

typedef struct fhe_ctx fhe_ctx;               /* device + stream (phantom::util::cuda_stream_wrapper, ntt_test.cu:40-41) */
typedef struct fhe_ntt_tables fhe_ntt_tables; /* DModulus[] + DNTTTable (ntt_test.cu:47-69) */
typedef struct fhe_baseconv fhe_baseconv;     /* base-conversion plan (rfhe_framewk/src/baseConv.py:14-18) */
typedef struct fhe_fourstep fhe_fourstep;     /* four-step plan (reliability_test/four_step_ntt_prot.py:71-79) */
typedef struct fhe_abft fhe_abft;             /* checksum weights of the ECC detector (rfhe_framewk/src/negaclic_ntt.py:130-149) */
typedef struct fhe_keyswitch fhe_keyswitch;   /* key-switch plan (shape of profile_framewk/build/data/ckks/16384_4:466-539) */

int fhe_version(void);
const char *fhe_last_error(void);

/* ---- context, memory, streams ------------------------------------------- */
/* cuda_stream_wrapper{ctor,get_stream} (ntt_test.cu:40-41).  device = HIP ordinal. */
int fhe_ctx_create(int device, fhe_ctx **out);
int fhe_ctx_destroy(fhe_ctx *ctx);
int fhe_ctx_stream(fhe_ctx *ctx, void **stream_out);
/* Tuning knobs (no reference counterpart): "ntt_mode" 0 = two launches per transform
 * (default), 1 = fused launch with the first-pass -> second-pass hand-off inside one XCD
 * (experimental, sizes 2^13..2^17); "fused_dist" pipeline distance between a limb's first
 * and second pass; "fused_wgs" persistent workgroups launched; "fused_variant" hand-off
 * load flavour; "ntt_resident" 1 = sizes 2^13 and 2^14 run as one LDS-resident pass
 * (their limb fits a CU's 160 KiB of LDS; experimental), 0 (default) = two launches like the larger sizes;
 * "ntt_packed" 1 = the forward 2^16 transform of FP64 limbs hands its intermediate over as packed 50-bit residues
 * (fewer bytes, more arithmetic: measured slower, experimental), 0 (default) = 8-byte words in place;
 * "ntt_chunk_mib" sub-batch size of two-launch transforms of batches above "ntt_chunk_floor_mib" (192) (default 96: a sub-batch's second launch finds
 * the first one's output in the 256 MiB Infinity Cache; 0 = one launch pair for the whole batch); "ntt_split" 1 / 0 / -1 = the
 * sub-batches of one call alternate between the caller's stream and a side stream the context owns, forked and joined by events
 * (one sub-batch's row pass runs under the next one's column pass; not inside a stream capture), -1 = default = on; "ntt_stream" 1 / 0 / -1 = non-temporal
 * loads / stores on the external side of the two launches (always / never / for sub-batched calls: the default); "ntt_pingpong" 1 / 0 / -1 = the two launches hand
 * over through a per-stream scratch buffer of one sub-batch, so that both run out of place (always / never / for calls that are
 * sub-batched: the default); "ks_fused" -1 / 0 / 1 = key-switch inner product
 * fused with the extended limbs' row pass by shape / never / always (hoisted batches of two or more elements transform the shared digits
 * once and use the plain inner product unless this is set); "hmult_fused_rescale" 1 (default) / 0 = fhe_hmult with rescale runs the mod-down and
 * the rescale behind one forward transform where the shape allows (two-launch sizes, K >= 2, no plain modulus) / as two steps (FHE_HMULT_FUSED_RESCALE);
 * "tile_geo" column-tile geometry of the two-launch path; "ntt_only_pass" 0 / 1 = launch only the
 * first / second pass of a two-pass size (timing of the individual kernels; -1 = whole transform).  Environment overrides at context creation: FHE_NTT_MODE=twopass|fused,
 * FHE_FUSED_DIST, FHE_FUSED_WGS.  Results are identical in every setting. */
int fhe_ctx_set_option(fhe_ctx *ctx, const char *name, long value);
/* Synchronises the streams used so far and reports whether any fused-NTT launch hit its
 * bounded-wait limit (never expected; the kernel then stops instead of hanging). */
int fhe_ctx_check(fhe_ctx *ctx);
/* cudaStreamSynchronize (ntt_test.cu:102,151) */
int fhe_sync(fhe_ctx *ctx, void *stream);
/* make_cuda_auto_ptr<uint64_t>(n, stream) / its destructor (ntt_test.cu:88) */
int fhe_alloc(fhe_ctx *ctx, size_t bytes, void **dptr);
int fhe_free(fhe_ctx *ctx, void *dptr);
/* cudaMemcpyAsync H2D / D2H / D2D (ntt_test.cu:89-101) */
int fhe_h2d(fhe_ctx *ctx, void *dst, const void *src, size_t bytes, void *stream);
int fhe_d2h(fhe_ctx *ctx, void *dst, const void *src, size_t bytes, void *stream);
int fhe_d2d(fhe_ctx *ctx, void *dst, const void *src, size_t bytes, void *stream);
int fhe_memset(fhe_ctx *ctx, void *dst, int byte, size_t bytes, void *stream);

/* ---- moduli and host tables (a10) ---------------------------------------- */
/* phantom::arith::CoeffModulus::Create(N, {bits...}) (ntt_test.cu:44): for each bit
 * size the largest primes p < 2^bits with p = 1 mod 2N, handed out smallest first.
 * N is a power of two, 1 <= N <= 2^59 (2N + 1, the smallest candidate, must stay below 2^61); bit sizes are in [2, 61], anything
 * else is FHE_ERR_UNSUPPORTED; a size whose interval (2^(bits-1), 2^bits) holds fewer such primes than the list asks for, a bad N
 * and count < 1 are FHE_ERR_INVALID. */
int fhe_moduli_create(uint64_t N, const int *bits, int count, uint64_t *out_q);
/* Modulus::const_ratio() (ntt_test.cu:51-52): out = {floor(2^128/q) lo, hi, 2^128 mod q} */
int fhe_modulus_const_ratio(uint64_t q, uint64_t out[3]);
/* minimal primitive `order`-th root of unity mod q (what phantom::arith::NTT picks).  q is a prime, `order` a power of two that
 * divides q - 1, at most 2^31 (the search for the minimum walks order / 2 products: seconds at the top); a larger order is
 * FHE_ERR_UNSUPPORTED, a composite q or an order that does not divide q - 1 FHE_ERR_INVALID. */
int fhe_min_primitive_root(uint64_t q, uint64_t order, uint64_t *out);
/* NTT::get_from_root_powers() / get_from_root_powers_shoup() (ntt_test.cu:60-64):
 * rp[bitrev(i)] = psi^i, shoup[k] = floor(rp[k] 2^64 / q); either pointer may be NULL */
int fhe_root_powers(uint64_t q, int log_n, uint64_t *rp, uint64_t *rp_shoup);

/* ---- NTT tables (device) -------------------------------------------------- */
/* DModulus::set + DNTTTable::init/set for `count` limbs (ntt_test.cu:47-69) with the
 * tables of phantom::arith::NTT(log_n, q[i]).  Limb i uses FHE_PATH_F64 when
 * q[i] < 2^50, else FHE_PATH_U64 (q[i] < 2^61).  Every q[i] is a prime that is 1 mod 2N, from the smallest such prime up:
 * q[i] >= 2^61 is FHE_ERR_UNSUPPORTED, a composite modulus or one without a 2N-th root FHE_ERR_INVALID. */
int fhe_ntt_tables_create(fhe_ctx *ctx, int log_n, const uint64_t *q, int count, fhe_ntt_tables **out);
/* Same, from caller-supplied forward root powers (count x N, entry k = psi^bitrev(k)):
 * the DNTTTable::set(..., twiddle, twiddle_shoup, ...) path of ntt_test.cu:61-69.
 * force_path: -1 = choose by modulus size, else FHE_PATH_*.  Either path takes every modulus below 2^50, however small;
 * FHE_PATH_F64 with q[i] >= 2^50 is FHE_ERR_UNSUPPORTED. */
int fhe_ntt_tables_create_from_roots(fhe_ctx *ctx, int log_n, const uint64_t *q, int count,
                                     const uint64_t *root_powers, int force_path, fhe_ntt_tables **out);
int fhe_ntt_tables_destroy(fhe_ntt_tables *t);
/* out_path[i] = arithmetic path of limb i; out_psi[i] = its 2N-th root (either may be NULL) */
int fhe_ntt_tables_info(const fhe_ntt_tables *t, int *log_n, int *count, int *out_path, uint64_t *out_psi);

/* ---- transforms (a2, a3) --------------------------------------------------- */
/* nwt_2d_radix8_forward_inplace(uint64_t*, const DNTTTable&, size_t coeff_modulus_size,
 * size_t start_modulus_idx, const cudaStream_t&) (ntt_test.cu:95,144; ntt_real_test.cu:89,126):
 * `limbs` forward negacyclic NTTs in place, limb i with modulus start_idx + i;
 * natural-order input, bit-reversed output, results in [0,q). */
int fhe_ntt_forward_inplace(fhe_ctx *ctx, uint64_t *d_data, const fhe_ntt_tables *t, size_t limbs, size_t start_idx,
                            void *stream);
/* Phantom's inverse (nwt_2d_radix8_backward_inplace, used inside multiply/decrypt,
 * reliability_test/dotprod_test.cu:113,119): bit-reversed input, natural output, times N^-1;
 * equals rfhe_framewk/src/negaclic_ntt.py:102-109 composed with the bit reversal. */
int fhe_ntt_inverse_inplace(fhe_ctx *ctx, uint64_t *d_data, const fhe_ntt_tables *t, size_t limbs, size_t start_idx,
                            void *stream);
/* Batched forms: d_data = [n_poly][limbs][N]; polynomial p, limb i uses modulus start_idx + i. */
int fhe_ntt_forward_batch(fhe_ctx *ctx, uint64_t *d_data, const fhe_ntt_tables *t, size_t n_poly, size_t limbs,
                          size_t start_idx, void *stream);
int fhe_ntt_inverse_batch(fhe_ctx *ctx, uint64_t *d_data, const fhe_ntt_tables *t, size_t n_poly, size_t limbs,
                          size_t start_idx, void *stream);

/* d_dst[v][i] = d_src[v][bitrev(i, log_n)] for n_vec vectors; d_dst != d_src.  Converts between
 * the bit-reversed order of the Phantom-style transforms and the natural order the
 * reference's Python returns (rfhe_framewk/src/negaclic_ntt.py:16-21,42). */
int fhe_bitrev_permute(fhe_ctx *ctx, uint64_t *d_dst, const uint64_t *d_src, int log_n, size_t n_vec, void *stream);

/* ---- cyclic transform (a1) --------------------------------------------------- */
/* ntt(a, mod, root) of motivation/ntt.py:8-32 (twins motivation/bsgs.py:5-29,
 * rfhe_framewk/src/ntt.py:38-55): natural order in and out, `root` a generator
 * (wlen = root^((mod-1)/len)); any modulus < 2^61, composite included.
 * convention 1 selects rfhe_framewk/src/negaclic_ntt.py:38-57 (root is a primitive
 * n-th root, wlen = root^(n/len)).  inverse != 0 gives intt(): transform with
 * root^(mod-2), then times n^(mod-2) (motivation/bsgs.py:31-36).
 * The result is that definition's for EVERY (mod, root), the degenerate ones included (n not dividing
 * mod - 1, an even modulus, a root that generates nothing: the exponents are rounded down as the
 * reference rounds them).  Where the stage roots form a tower -- wlen(2) = -1, wlen(2 len)^2 = wlen(len),
 * a sufficient condition, applied conservatively -- lengths from 2^5 run as the two natural-order launches;
 * every other call runs the forward network with the same table and a bit-reversal gather (three
 * launches), which is the definition itself relabelled.  The operation trace names the route taken
 * (NTT_CYCLIC_NATURAL_ORDER / NTT_CYCLIC_FORWARD_NETWORK).
 * d_data: n_vec vectors of 2^log_n words, in place; d_scratch: same size. */
int fhe_ntt_cyclic(fhe_ctx *ctx, uint64_t *d_data, uint64_t *d_scratch, int log_n, size_t n_vec, uint64_t mod,
                   uint64_t root, int convention, int inverse, void *stream);

/* ---- four-step transform (a6) -------------------------------------------------- */
/* four_step_ntt(a, N) of reliability_test/four_step_ntt_prot.py:71-109 with N = n1*n2
 * (both powers of two, n1 != n2 allowed): column transforms, twiddle w^(k2 t1), row
 * transforms, transposed output; equals ntt_direct (:49-58).  g = generator (G=3, :17): fhe_fourstep_create
 * returns FHE_ERR_INVALID unless N divides mod - 1 and w = g^((mod-1)/N) has w^(N/2) = -1 (g a quadratic
 * non-residue of a prime modulus), the plans on which the engine's network is that direct DFT. */
/* Range: 2 <= n1, n2 <= 2^20, n1 * n2 <= 2^26, mod < 2^61 (FHE_ERR_INVALID / FHE_ERR_UNSUPPORTED beyond).  Up to N = 2^20 the whole flow
 * is ONE natural-order transform of the engine (two launches, no transpose pass); from 2^21 to 2^26 (the reference's default modulus
 * 998244353 admits N up to 2^23) it is the reference's composition itself: transpose, n1 transforms of length n2, the twiddle on the
 * way through the second transpose, n2 transforms of length n1, transpose -- five sweeps, plan-owned buffers of two batches.
 * A plan's hand-off buffers are reused by every call on it: one plan, one stream at a time (see fhe_hmult). */
int fhe_fourstep_create(fhe_ctx *ctx, uint64_t n1, uint64_t n2, uint64_t mod, uint64_t g, fhe_fourstep **out);
int fhe_fourstep_destroy(fhe_fourstep *p);
int fhe_fourstep_ntt(fhe_ctx *ctx, uint64_t *d_dst, const uint64_t *d_src, fhe_fourstep *p, void *stream);
/* n_vec vectors of n1*n2 words each, contiguous; d_dst may equal d_src.  Two launches for the whole batch: the column
 * transforms read the input's columns directly (no transpose pass), the row transforms carry the twiddle step in their
 * butterflies and write natural order. */
int fhe_fourstep_ntt_batch(fhe_ctx *ctx, uint64_t *d_dst, const uint64_t *d_src, fhe_fourstep *p, size_t n_vec, void *stream);
/* ABFT-checked four-step transform (four_step_with_protection_vector, reliability_test/four_step_ntt_prot.py:185-252, which checks
 * its two stages with sum(C) == col_sums(A) . row_sums(B) and reports stage1 / stage2).  The words written are those of
 * fhe_fourstep_ntt_batch, bit for bit; the weighted checksums ride on the two launches (no extra sweep over the data):
 *   v_kappa = (kappa mod 2^(logN/2) + 1) + (kappa div 2^(logN/2) + 1) on the natural-order output (generate_weights,
 *   rfhe_framewk/src/negaclic_ntt.py:7-13 -- not the reference's all-ones weights, which weigh x_0 only), u = W v on the input,
 *   m = (launch 2)^T v on the hand-off words between the launches; per vector
 *     launch 1: sum u x == sum m z,   hand-off: sum m z as stored == as loaded,   launch 2: sum m z == sum v y.
 * Not covered: faults already in the input, a fault between a tap's read of a register and the instruction that consumes it, a wrong
 * plan handed in by the caller.  A fault e at a word is invisible exactly when e * weight == 0 modulo `mod`: preparation fails with
 * FHE_ERR_UNSUPPORTED (naming the table and the index) when an entry of u, m or v is 0 modulo `mod` -- tiny moduli do this.
 * Plans past N = 2^20 return FHE_ERR_UNSUPPORTED; n_vec == 0 returns FHE_OK and touches nothing; d_dst may equal d_src.  Batches
 * that fhe_fourstep_ntt_batch cuts are cut the same way (never while a test hook is armed).
 * _prepare_checked builds the weight tables (one unchecked transform of v and one column pass); the other calls run it on first
 * use, except inside a stream capture, where they return FHE_ERR_INVALID when the tables (or the batch's scratch) are missing.
 * _checksum: d_out[vector] = sum u x (side 0, d_data = input vectors) or sum v y (side 1, d_data = output vectors) modulo `mod`.
 * _ntt_checked: d_flags = one uint32 per vector (0 / 1), sum u x != sum v y; N = 2 .. 2^20 (below 32: separate reduction launches).
 * _ntt_checked_phases: d_flags = [n_vec][3], launch 1 / hand-off / launch 2; N >= 2^13, FHE_ERR_UNSUPPORTED below.
 * Test hooks (no setter of their own): fhe_ctx_inject_fault(idx, bit) flips word idx of the hand-off buffer [n_vec][N] between the
 * two launches; fhe_ctx_inject_fault_in_pass(pass, workgroup, lds_word, bit) flips a word of that workgroup's LDS image between the
 * first two register steps of launch `pass` (per-phase call only).  Both are read and disarmed by either checked call whatever its
 * outcome; a call without such a point (single-launch sizes, the in-pass hook on the whole-transform call) returns
 * FHE_ERR_UNSUPPORTED, an index outside the call's window FHE_ERR_INVALID, before anything is launched. */
int fhe_fourstep_prepare_checked(fhe_ctx *ctx, fhe_fourstep *p, void *stream);
int fhe_fourstep_checksum(fhe_ctx *ctx, fhe_fourstep *p, int side, const uint64_t *d_data, uint64_t *d_out, size_t n_vec, void *stream);
int fhe_fourstep_ntt_checked(fhe_ctx *ctx, uint64_t *d_dst, const uint64_t *d_src, fhe_fourstep *p, size_t n_vec, uint32_t *d_flags, void *stream);
int fhe_fourstep_ntt_checked_phases(fhe_ctx *ctx, uint64_t *d_dst, const uint64_t *d_src, fhe_fourstep *p, size_t n_vec, uint32_t *d_flags,
                                    void *stream);

/* ---- coefficient-wise products (a4, a5) ------------------------------------------ */
/* C_hat[i] = A_hat[i] * B_hat[i] % mod (rfhe_framewk/src/negaclic_ntt.py:126), per limb;
 * the NTT-domain core of phantom::multiply (dotprod_test.cu:113).  c may alias a or b. */
int fhe_modmul(fhe_ctx *ctx, uint64_t *d_c, const uint64_t *d_a, const uint64_t *d_b, const fhe_ntt_tables *t,
               size_t n_poly, size_t limbs, size_t start_idx, void *stream);
/* c = (c + a*b) mod q: keyswitch / BSGS inner-product accumulate (motivation/bsgs.py:50) */
int fhe_modmul_acc(fhe_ctx *ctx, uint64_t *d_c, const uint64_t *d_a, const uint64_t *d_b, const fhe_ntt_tables *t,
                   size_t n_poly, size_t limbs, size_t start_idx, void *stream);
/* c = (a + b) mod q per limb (phantom::add_inplace, reliability_test/dotprod_test.cu:147); fhe_modsub: c = (a - b) mod q.
 * Operands need not be canonical: any 64-bit word stands for its residue modulo q_l, the result is in [0, q_l).  Buffers are
 * [n_poly][limbs][N] (dense in the window's limbs when start_idx > 0); c may alias a or b, and a may alias b. */
int fhe_modadd(fhe_ctx *ctx, uint64_t *d_c, const uint64_t *d_a, const uint64_t *d_b, const fhe_ntt_tables *t, size_t n_poly,
               size_t limbs, size_t start_idx, void *stream);
int fhe_modsub(fhe_ctx *ctx, uint64_t *d_c, const uint64_t *d_a, const uint64_t *d_b, const fhe_ntt_tables *t, size_t n_poly,
               size_t limbs, size_t start_idx, void *stream);
/* c = a * mul[l] + add[l] mod q_l with one host-side scalar pair per limb (either array may be NULL:
 * mul defaults to 1, add to 0); limbs <= 64, more is FHE_ERR_UNSUPPORTED with nothing launched.  Neither the words of a nor the
 * scalars need be canonical: any 64-bit value stands for its residue modulo q_l (the scalars are reduced on the host, the words in
 * the kernel), so with both arrays NULL the call is c = a mod q.  The result is in [0, q_l); c may alias a.  Scalar steps of
 * mod-switching and BGV decryption
 * (phantom::mod_switch_to_next_inplace / PhantomSecretKey::decrypt, dotprod_test.cu:115,119). */
int fhe_scalar_affine(fhe_ctx *ctx, uint64_t *d_c, const uint64_t *d_a, const uint64_t *mul, const uint64_t *add,
                      const fhe_ntt_tables *t, size_t n_poly, size_t limbs, size_t start_idx, void *stream);
/* poly_mul_negacyclic_ntt (rfhe_framewk/src/negaclic_ntt.py:123-127): c = a * b mod (x^N + 1, q).
 * a and b are scratch: their contents are unspecified afterwards (partly transformed); c may alias
 * either.  One read of each factor tile and one write of the product tile between the column passes. */
int fhe_polymul(fhe_ctx *ctx, uint64_t *d_c, uint64_t *d_a, uint64_t *d_b, const fhe_ntt_tables *t, size_t n_poly,
                size_t limbs, size_t start_idx, void *stream);

/* ---- base conversion / CRT (a8) ------------------------------------------------- */
int fhe_baseconv_create(fhe_ctx *ctx, const uint64_t *mod_in, int m, const uint64_t *mod_out, int k,
                        fhe_baseconv **out);
int fhe_baseconv_destroy(fhe_baseconv *p);
/* base_conv_fixed (motivation/baseConv.py:67-83): exact; in m x N, out k x N (limb-major) */
int fhe_baseconv_exact(fhe_ctx *ctx, uint64_t *d_out, const uint64_t *d_in, const fhe_baseconv *p, size_t N,
                       void *stream);
/* bConv (rfhe_framewk/src/baseConv.py:10-40): sum_j ((r_j Phat_j inv_j) mod q_k), NOT reduced;
 * out k x N limb-major (the reference returns the transposed [i][k] list).  Requires
 * m * max(q_k) < 2^64. */
int fhe_baseconv_fast(fhe_ctx *ctx, uint64_t *d_out, const uint64_t *d_in, const fhe_baseconv *p, size_t N,
                      void *stream);
/* crt_kernel (rfhe_framewk/src/baseConv.cu:85-120, launch :187-193): Garner CRT of m <= 16
 * limbs into a 128-bit integer (lo, hi) per coefficient, 128-bit wrap-around as the
 * kernel; residues m x N row-major. */
int fhe_crt_garner(fhe_ctx *ctx, uint64_t *d_x_lo, uint64_t *d_x_hi, const uint64_t *d_residues,
                   const uint64_t *moduli, int m, size_t N, void *stream);

/* ---- BSGS block-diagonal Hadamard (a9) --------------------------------------------- */
/* diag_block_hadamard_matvec (motivation/bsgs.py:39-52): y_i = sum_j M[(j-i) mod k] (.) v_j,
 * k blocks of `block_size`.  mod == 0: int64 wrap-around, no reduction (the reference's
 * NumPy arithmetic); otherwise every product and the sum are reduced mod `mod`. */
int fhe_bsgs_hadamard(fhe_ctx *ctx, uint64_t *d_y, const uint64_t *d_M_blocks, const uint64_t *d_v, int k,
                      int block_size, uint64_t mod, void *stream);

/* ---- rotation / key switching ----------------------------------- */
/* Galois automorphism x -> x^galois_elt (odd) -- the index map behind phantom::rotate_inplace
 * (reliability_test/dotprod_test.cu:146) -- on coefficient-domain limbs: dst[(i k) mod N] = +-src[i].
 * d_dst != d_src; layout [n_poly][limbs][N]. */
int fhe_automorphism(fhe_ctx *ctx, uint64_t *d_dst, const uint64_t *d_src, const fhe_ntt_tables *t, uint32_t galois_elt,
                     size_t n_poly, size_t limbs, size_t start_idx, void *stream);
/* The same map on NTT-domain limbs (bit-reversed order): a pure permutation of the slots. */
int fhe_automorphism_ntt(fhe_ctx *ctx, uint64_t *d_dst, const uint64_t *d_src, int log_n, uint32_t galois_elt, size_t n_units,
                         void *stream);
/* Hybrid RNS key switching with the operation sequence the reference's SEAL trace shows for one
 * KEYSWITCH + MODSWITCH (profile_framewk/build/data/ckks/16384_4:466-539; summary in
 * profile_framewk/build/sum_trace.py:10-94): INTT of the input limbs, per digit base extension to every
 * other prime ("MODREDUCTION"), NTT, multiply-accumulate with the evaluation key ("MULTEVALK"), then
 * mod-down by the special primes (INTT, conversion, NTT, subtract, times P^-1).
 * `t` holds L ciphertext primes followed by K special primes; the L primes are cut into `dnum` digits of
 * ceil(L/dnum) consecutive limbs (SEAL: dnum = L, one prime per digit; draw_dnum_rot_mul.py:64 sweeps dnum).
 *   d_c   : L x N, NTT domain                       d_evk : dnum x 2 x (L+K) x N, NTT domain (b_d, a_d)
 *   d_out0, d_out1 : L x N, NTT domain; out0 + out1*s ~ c*s' when evk encrypts P*Qhat_d*[Qhat_d^-1]_{Q_d}*s'.
 * The plan owns the intermediate buffers (extended digits, accumulators): one call at a time per plan. */
int fhe_keyswitch_create(fhe_ctx *ctx, const fhe_ntt_tables *t, int L, int K, int dnum, fhe_keyswitch **out);
/* The same key switch with the RNS limbs sharded over `world` ranks, one process per GPU (BASELINE configs 4-5; the reference
 * has no multi-device code).  Rank r owns the ciphertext limbs [clo, clo+cn) and the special limbs
 * [slo, slo+sn) that fhe_keyswitch_shard_layout reports (out = {clo, cn, slo, sn, cmax, smax}; pure host function, no
 * device needed): its rows of the input (cn x N), of every key digit (dnum x 2 x (cn+sn) x N, ciphertext rows first) and of
 * the result.  The only exchanges are two all-gathers, issued by the host between the three phases (RCCL over xGMI when
 * the host uses torch.distributed's "nccl" backend):
 *   fhe_keyswitch_shard_begin   INTT of the owned input limbs into rows [rank*cmax, rank*cmax+cn) of d_gather1
 *   -- all-gather of d_gather1 ([world][cmax][N] words, in place) --
 *   fhe_keyswitch_shard_inner   digit extension to the owned limbs, NTT, inner product with the owned key rows, INTT of
 *                               the owned special limbs of both halves into slot `rank` of d_gather2 ([world][2][smax][N])
 *   -- all-gather of d_gather2 (in place) --
 *   fhe_keyswitch_shard_finish  mod-down to the owned ciphertext limbs (+ optional addends, as a rotation / relinearisation needs)
 * The gather buffers belong to the caller and are fixed at creation.  world = 1 gives fhe_keyswitch_create's plan.
 * d_bcast (optional, 3 x N words): broadcast buffer of the sharded rescale below; NULL = the plan does not rescale. */
int fhe_keyswitch_shard_layout(int L, int K, int world, int rank, int out[6]);
int fhe_keyswitch_create_sharded(fhe_ctx *ctx, const fhe_ntt_tables *t, int L, int K, int dnum, int world, int rank,
                                 uint64_t *d_gather1, uint64_t *d_gather2, uint64_t *d_bcast, fhe_keyswitch **out);
int fhe_keyswitch_shard_begin(fhe_ctx *ctx, fhe_keyswitch *p, const uint64_t *d_c_local, void *stream);
int fhe_keyswitch_shard_inner(fhe_ctx *ctx, fhe_keyswitch *p, const uint64_t *d_c_local, const uint64_t *d_evk_local, void *stream);
int fhe_keyswitch_shard_finish(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0_local, uint64_t *d_out1_local,
                               const uint64_t *d_add0_local, const uint64_t *d_add1_local, void *stream);
/* BGV form of the mod-down: with plaintext modulus `plain_modulus` (0 = off, the CKKS-style flooring
 * above) the removed part delta satisfies delta = acc mod P and delta = 0 mod plain_modulus, so the
 * plaintext is preserved exactly (scheme of reliability_test/dotprod_test.cu:199-204). */
int fhe_keyswitch_set_plain_modulus(fhe_keyswitch *p, uint64_t plain_modulus);
/* Rounding of every rescale the plan runs: mode 0 = floor (the default), 1 = round to nearest (fhe_rescale below gives both
 * definitions).  Honoured by fhe_rescale, fhe_hmult with rescale != 0 on both of its routes, fhe_rescale_shard_begin / _finish and
 * fhe_hmult_shard_finish_begin / _end (every rank sets the same mode).  Host state only; mode 0 restores every launch list and word.
 * The mod-down inside the key switch floors in either mode.  Refusals: another mode FHE_ERR_INVALID; mode 1 on a plan with a plain
 * modulus, and a plain modulus on a plan in mode 1, FHE_ERR_UNSUPPORTED (the BGV mod switch removes t [c t^-1] -- another operation).
 * On a plan in mode 1 every checked, sealed or repairing call that would drop a prime -- fhe_rescale_checked, fhe_rescale_sealed,
 * fhe_hmult_checked / _sealed / _sealed_fused / _sealed_fused_key / _sealed_out / _sealed_repair with rescale != 0 -- returns
 * FHE_ERR_UNSUPPORTED after taking its one-shot hooks, with nothing launched: they restate the flooring form. */
int fhe_keyswitch_set_rescale_rounding(fhe_keyswitch *p, int mode);
int fhe_keyswitch_get_rescale_rounding(const fhe_keyswitch *p, int *mode);
int fhe_keyswitch_destroy(fhe_keyswitch *p);
int fhe_keyswitch_apply(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c,
                        const uint64_t *d_evk, void *stream);

/* Rotation of a two-part ciphertext (c0, c1), NTT domain, L limbs each -- phantom::rotate_inplace
 * (dotprod_test.cu:146), frontend "ROTATE" of the reference's traces (16384_4:466-539): apply
 * x -> x^galois_elt to both parts, key-switch the second part with the Galois key, add.
 * out0 + out1*s ~ sigma(c0 + c1*s). */
/* OUT OF PLACE: the parts are read through the Galois permutation while the outputs are written -- neither output may be one of the
 * input parts (FHE_ERR_INVALID); the same holds for fhe_rotate_shard_finish's d_c0_local. */
int fhe_rotate(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1,
               uint32_t galois_elt, const uint64_t *d_galois_key, void *stream);
/* Hoisted rotations: n_rot rotations of ONE ciphertext (the baby steps of a BSGS matrix-vector product,
 * profile_framewk/src/matmul_ckks.cpp:45-113; rotate-and-sum, reliability_test/dotprod_test.cu:143-148).  The decomposition of c1 --
 * INTT, digit extension, the extended limbs' forward transform -- is shared; per Galois element only the inner product with the key
 * and the mod-down run (sigma is taken on the mod-down's loads).  Keys are given in the UN-ROTATED frame:
 * d_prepared_keys[r] = fhe_galois_key_prepare(key of galois_elts[r]) = sigma^-1 of every key row, computed once per key (layout
 * unchanged, [dnum][2][L+K][N]).  d_out0 / d_out1 / d_prepared_keys are HOST arrays of n_rot device pointers.
 * Each result is a rotation of (c0, c1) by its element -- out0 + out1 s ~ sigma(c0 + c1 s) -- with ext_d = sigma(extension of c1's
 * digit); fhe_rotate extends sigma(c1)'s digit instead, so the two differ word by word (by multiples of the digit moduli where sigma
 * flips a sign) while decrypting to the same plaintext.  One device, N >= 2^5, out of place. */
int fhe_galois_key_prepare(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_key_out, const uint64_t *d_key_in, uint32_t galois_elt, void *stream);
int fhe_rotate_hoisted(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *const *d_out0, uint64_t *const *d_out1, const uint64_t *d_c0,
                       const uint64_t *d_c1, const uint32_t *galois_elts, const uint64_t *const *d_prepared_keys, size_t n_rot, void *stream);
/* Hoisted rotations with the limbs sharded (plans of fhe_keyswitch_create_sharded): gather 1 and the digit extension are shared by all
 * elements, so a rotation costs ONE all-gather (the special limbs') instead of two.  Per ciphertext: _begin (INTT of the owned limbs of the
 * un-rotated c1 into d_gather1), all-gather of d_gather1, _extend; per Galois element: _inner (inner product with the owned rows of the
 * prepared key -- fhe_galois_key_prepare on the rank's rows --, INTT of sigma(owned special limbs) into d_gather2), all-gather of d_gather2,
 * _finish (mod-down to the owned limbs; sums and c0 read through the Galois map).  Values as fhe_rotate_hoisted. */
int fhe_rotate_hoisted_shard_begin(fhe_ctx *ctx, fhe_keyswitch *p, const uint64_t *d_c1_local, void *stream);
int fhe_rotate_hoisted_shard_extend(fhe_ctx *ctx, fhe_keyswitch *p, void *stream);
int fhe_rotate_hoisted_shard_inner(fhe_ctx *ctx, fhe_keyswitch *p, const uint64_t *d_c1_local, const uint64_t *d_prepared_key_local,
                                   uint32_t galois_elt, void *stream);
int fhe_rotate_hoisted_shard_finish(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0_local, uint64_t *d_out1_local, const uint64_t *d_c0_local,
                                    uint32_t galois_elt, void *stream);
/* Baby-step / giant-step matrix-vector product on a two-part ciphertext x = (c0, c1) (profile_framewk/src/matmul_ckks.cpp:45-113 --
 * rotate, multiply_plain with a diagonal, add -- in the arrangement with n1 + n2 - 2 rotations; plaintext block form:
 * motivation/bsgs.py:39-52):
 *     y = sum_{g < n2} sigma_{giant_elts[g-1]}( sum_{b < n1} diag[g][b] (.) sigma_{baby_elts[b-1]}(x) ),   g = 0 and b = 0: no rotation.
 * d_diags = [n2][n1][L][N] NTT-form plaintext polynomials (the caller pre-rotates the diagonals of giant step g by -g n1, as BSGS
 * requires); baby keys in the un-rotated frame (fhe_galois_key_prepare), giant keys as fhe_rotate takes them; baby_elts / the key
 * arrays have n1 - 1 resp. n2 - 1 entries (host arrays).  The n1 - 1 baby rotations share one decomposition of x
 * (fhe_rotate_hoisted), each inner sum is one launch, the giant rotations are fhe_rotate calls accumulated into (d_out0, d_out1).
 * No rescale inside (apply fhe_rescale to the result).  Out of place; one device. */
int fhe_bsgs_matvec(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1,
                    const uint64_t *d_diags, size_t n1, size_t n2, const uint32_t *baby_elts, const uint64_t *const *d_baby_keys_prepared,
                    const uint32_t *giant_elts, const uint64_t *const *d_giant_keys, void *stream);
/* The same rotation on a limb-sharded plan (fhe_keyswitch_create_sharded): the automorphism permutes slots inside a limb, so each
 * rank applies it to its own rows -- on the loads of the launches below, there is no permuted copy of c0 and no launch for it.
 * Phases and joins as for the sharded key switch:
 *   fhe_rotate_shard_begin   INTT of sigma(c1)'s owned limbs into this rank's rows of d_gather1   -- all-gather of d_gather1 --
 *   fhe_rotate_shard_inner   extension, NTT, inner product with the owned Galois-key rows, INTT of the owned special limbs
 *                            -- all-gather of d_gather2 --
 *   fhe_rotate_shard_finish  mod-down to the owned limbs, sigma(c0) added to the first part */
int fhe_rotate_shard_begin(fhe_ctx *ctx, fhe_keyswitch *p, const uint64_t *d_c1_local, uint32_t galois_elt, void *stream);
int fhe_rotate_shard_inner(fhe_ctx *ctx, fhe_keyswitch *p, const uint64_t *d_galois_key_local, void *stream);
int fhe_rotate_shard_finish(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0_local, uint64_t *d_out1_local, const uint64_t *d_c0_local,
                            uint32_t galois_elt, void *stream);
/* ---- homomorphic multiply: tensor product, relinearisation, rescale (BASELINE config 4) -------------- */
/* phantom::multiply (reliability_test/dotprod_test.cu:113; frontend MULTIPLY_CKKS of the SEAL traces,
 * profile_framewk/build/data/ckks/16384_4:388-389): per limb d0 = a0 b0, d1 = a0 b1 + a1 b0, d2 = a1 b1 on NTT-form
 * parts of `limbs` limbs each, one pass over the seven operands. */
int fhe_tensor_product(fhe_ctx *ctx, uint64_t *d_d0, uint64_t *d_d1, uint64_t *d_d2, const uint64_t *d_a0, const uint64_t *d_a1,
                       const uint64_t *d_b0, const uint64_t *d_b1, const fhe_ntt_tables *t, size_t limbs, size_t start_idx, void *stream);
/* phantom::relinearize_inplace (dotprod_test.cu:114; frontend RELIN, 16384_4:390-451): (d0, d1, d2) -> (d0 + ks0, d1 + ks1)
 * with (ks0, ks1) = key switch of d2 under the relinearisation key (layout of fhe_keyswitch_apply's d_evk); the two
 * additions ride on the key switch's last launch. */
int fhe_relinearize(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_d0, const uint64_t *d_d1,
                    const uint64_t *d_d2, const uint64_t *d_relin_key, void *stream);
/* phantom::mod_switch_to_next_inplace (dotprod_test.cu:115) / CKKS rescale: drop the plan's last ciphertext prime on each of
 * n_parts (1..3) parts; d_in = [n_parts][L][N], d_out = [n_parts][L-1][N], NTT domain.  Two roundings, chosen per plan
 * (fhe_keyswitch_set_rescale_rounding below), with C in [0, Q) the CRT lift of a coefficient, q = q_last, h = (q - 1) / 2:
 *   mode 0, floor (the default):  c' = (C - [C]_q) / q,  [C]_q in [0, q);
 *   mode 1, nearest:              c' = floor((C + h) / q) = (C - r) / q,  r = [C]_q if [C]_q <= h else [C]_q - q  (q is odd: no ties)
 *                                 -- SEAL's rescale_to_next_inplace (RNSTool::divide_and_round_q_last_ntt_inplace).
 * Output limb j is the canonical word of NTT_j((c_j - (r mod q_j)) q^-1 mod q_j).  The nearest form is pinned by this integer
 * definition (tests/helpers/rescale_round.py); its word-for-word parity with a SEAL or Phantom build is unpinned -- neither is at hand.
 * With a plain modulus set on the plan (BGV) the removed part is t [c t^-1]_{q_last}, so the plaintext is kept up to the factor
 * q_last^-1 mod t; that form has no rounding mode. */
/* OUT OF PLACE: input parts are L rows apart, output parts L-1 -- d_out must not overlap d_in (FHE_ERR_INVALID). */
int fhe_rescale(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out, const uint64_t *d_in, size_t n_parts, void *stream);
/* fhe_rescale with the limbs sharded (plans of fhe_keyswitch_create_sharded with a d_bcast buffer): d_in_local = [n_parts][cn][N], the
 * rows this rank owns.  _begin: the owner of limb L-1 (fhe_rescale_shard_info: owns_last) turns the last limb of every part to
 * coefficient form into d_bcast; the host broadcasts d_bcast from that rank (n_parts x N words, the one exchange); _finish: every
 * rank forms (c - delta) / q_last on the out_rows owned limbs below L-1, d_out_local = [n_parts][out_rows][N]. */
int fhe_rescale_shard_info(const fhe_keyswitch *p, int *owns_last, int *out_rows);
int fhe_rescale_shard_begin(fhe_ctx *ctx, fhe_keyswitch *p, const uint64_t *d_in_local, size_t n_parts, void *stream);
int fhe_rescale_shard_finish(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out_local, const uint64_t *d_in_local, size_t n_parts, void *stream);
/* The three steps above in one call (multiply -> relinearize -> mod_switch, dotprod_test.cu:113-115) on two two-part
 * ciphertexts of L limbs; rescale != 0: outputs have L-1 limbs, else L.  The plan owns the intermediates. */
/* The operands are consumed by the first launch (tensor product into plan-owned buffers), so an output may reuse an operand's
 * buffer; d_out0 and d_out1 must be distinct.
 * ONE PLAN, ONE STREAM AT A TIME: a plan (fhe_keyswitch, fhe_fourstep, fhe_abft) owns scratch buffers -- extended digits, sums,
 * converted limbs, the tensor product, rescale residues, the four-step hand-off, checksum partials -- that every call on it
 * reuses.  Calls on the SAME plan must be ordered by one stream (or by the caller's events); different plans, and the plan-less
 * transforms / products, may run on different streams concurrently. */
int fhe_hmult(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_a0, const uint64_t *d_a1,
              const uint64_t *d_b0, const uint64_t *d_b1, const uint64_t *d_relin_key, int rescale, void *stream);
/* multiply -> relinearize -> mod_switch with the limbs sharded, the mod-down and the rescale behind ONE forward transform (what
 * fhe_hmult does on one device where fhe_hmult_shard_fusable() / the shape allow: two-launch sizes, K >= 2, CKKS form): after
 * fhe_tensor_product, fhe_keyswitch_shard_begin / _inner and their two all-gathers,
 *   _finish_begin: converts the gathered special limbs to this rank's rows; the owner of limb L-1 writes
 *                  y = INTT(v_{L-1}) of both parts into d_bcast ([2][N] of it), d_add*_local = this rank's rows of d0 / d1;
 *   the host broadcasts d_bcast from that rank (the one exchange of the rescale);
 *   _finish_end:   d_out*_local = [out_rows][N] (fhe_rescale_shard_info), the owned limbs below L-1 of the rescaled parts.
 * Same words as fhe_keyswitch_shard_finish + fhe_rescale_shard_begin / _finish (reliability_test/dotprod_test.cu:114-115). */
int fhe_hmult_shard_fusable(const fhe_ctx *ctx, const fhe_keyswitch *p);
int fhe_hmult_shard_finish_begin(fhe_ctx *ctx, fhe_keyswitch *p, const uint64_t *d_add0_local, const uint64_t *d_add1_local, void *stream);
int fhe_hmult_shard_finish_end(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0_local, uint64_t *d_out1_local, const uint64_t *d_add0_local,
                               const uint64_t *d_add1_local, void *stream);

/* Operation trace in the line format the reference's tools consume
 * (profile_framewk/build/analyze_trace.py:16-19, sum_trace.py:16-19): "frontend: ROTATE",
 * "[NTT] total cost <n> us" per transform launch, "[MODREDUCTION]/[MULTEVK]/[KEYSWITCH]/[MODSWITCH] total
 * cost <n> us" (inclusive of the transforms before them, as SEAL's timers are), "frontend: ROTATE[<n>
 * microseconds]".  While enabled every traced step synchronises the stream (timing tool, not a fast
 * path).  fhe_ctx_trace_read copies the text collected so far (NUL-terminated, truncated to `cap`) and
 * returns its full length through *len. */
int fhe_ctx_trace(fhe_ctx *ctx, int enable);
int fhe_ctx_trace_read(fhe_ctx *ctx, char *buf, size_t cap, size_t *len);

/* ---- ABFT detector around the forward NTT, the inverse NTT and the product ---- */
/* Weighted-checksum ECC of rfhe_framewk/src/negaclic_ntt.py:130-149: with weights w (generate_weights,
 * :7-13: w[i] = (i % p + 1) + (i / p + 1), p = 2^floor(log_n / 2)) and w_hat = V^-T w, a correct
 * transform satisfies sum_i w_i a_i = sum_j w_hat_j a_hat_j (mod q).  w_hat is obtained on the device
 * from the forward transform itself: w_hat = N^-1 * NTT(w_0, -w_{N-1}, ..., -w_1), already in the
 * engine's bit-reversed order.  One weight set per limb of `t`.  The same two sets check the inverse transform (sides swapped)
 * and the product (sum w c = sum w_hat a_hat b_hat).  Not covered: faults already in the input, and a register fault between
 * a checksum's read of a value and the instruction that consumes the same register. */
int fhe_abft_create(fhe_ctx *ctx, const fhe_ntt_tables *t, fhe_abft **out);
int fhe_abft_destroy(fhe_abft *a);
/* side 0: d_out[unit] = sum_i w_i x_i (input side); side 1: N^-1 sum_j w'_j x_j (output side) */
int fhe_abft_checksum(fhe_ctx *ctx, const fhe_abft *a, int side, const uint64_t *d_data, uint64_t *d_out, size_t n_poly,
                      size_t limbs, size_t start_idx, void *stream);
/* Forward NTT with the detector around it: d_flags[unit] (uint32) = 1 where the two checksums differ,
 * i.e. where a fault hit the transform of that limb-polynomial (faults already present in the input
 * are, by construction, not flagged).  For N >= 32 the two checksums are accumulated inside the
 * transform's own passes (from the registers just loaded / the words about to be stored): no extra
 * sweep over the data.  The detector object owns scratch: one call at a time per fhe_abft. */
int fhe_ntt_forward_checked(fhe_ctx *ctx, uint64_t *d_data, const fhe_ntt_tables *t, const fhe_abft *a, size_t n_poly,
                            size_t limbs, size_t start_idx, uint32_t *d_flags, void *stream);
/* The same detector phase by phase, where the reference checks its four-step flow: batch_check of the column transforms,
 * check_inter around the twiddle step, batch_check of the row transforms (rfhe_framewk/src/ntt_test/relia_ntt_sim.cpp:235-292,
 * 331-355; the per-multiply equality of reliability_test/four_step_ntt_prot.py:185-194).  The engine's two launches are that
 * flow (column transforms; row transforms with the twiddle folded into their butterflies), so three flags per
 * limb-polynomial, d_flags[3*unit + k]:
 *   k = 0  column pass : sum w x over the words it loaded  !=  sum u y over the words it stored       (u = P1^-T w)
 *   k = 1  hand-off    : sum u y as stored by the column pass  !=  as loaded by the row pass (corruption between the launches)
 *   k = 2  row pass    : sum u y over the words it loaded  !=  sum w^ X over the words it stored
 * A fault raises the flag of the phase it hit and no other.  Two-launch sizes (N >= 2^13); smaller transforms are one
 * launch = one phase: fhe_ntt_forward_checked. */
int fhe_ntt_forward_checked_phases(fhe_ctx *ctx, uint64_t *d_data, const fhe_ntt_tables *t, const fhe_abft *a, size_t n_poly,
                                   size_t limbs, size_t start_idx, uint32_t *d_flags, void *stream);
/* Inverse NTT with the detector around it: the same two weight sets with the sides swapped (x = F^-1 x_hat gives
 * sum_j w_hat_j x_hat_j = sum_i w_i x_i).  d_flags[unit] = 1 where the input-side sum (w_hat, over the words the first launch
 * loads) differs from the output-side sum (w, over the words the last launch stores).  The output words are those of
 * fhe_ntt_inverse_inplace, bit for bit.  Same sizes, arithmetic paths, limb windows and sub-batches as the forward detector;
 * fhe_ctx_inject_fault flips a word between the row pass and the column pass (N >= 2^13). */
int fhe_ntt_inverse_checked(fhe_ctx *ctx, uint64_t *d_data, const fhe_ntt_tables *t, const fhe_abft *a, size_t n_poly,
                            size_t limbs, size_t start_idx, uint32_t *d_flags, void *stream);
/* fhe_polymul with the detector (the protected chain transform -> element-wise product -> transform of
 * rfhe_framewk/src/four_step_ntt_protected.py:219-282).  Same contract as fhe_polymul: a and b are scratch, c may alias either,
 * the product words are fhe_polymul's.  Three flags per limb-polynomial, d_flags[3*unit + k]:
 *   k = 0  forward transform of a : sum w a over the loaded words  !=  sum w_hat a_hat as the product consumes a_hat
 *   k = 1  the same for b (for a == b it equals k = 0)
 *   k = 2  product, hand-off and inverse : sum w_hat a_hat b_hat (formed next to the product, not from its result)  !=  sum w c
 *          over the stored result   (c_hat_j = a_hat_j b_hat_j gives sum_i w_i c_i = sum_j w_hat_j a_hat_j b_hat_j)
 * For N >= 2^5 the sums ride on the product's own launches (no extra sweep over the data); smaller sizes and the fused-NTT mode
 * use separate reductions.  Faults already present in a or b are not flagged, and neither is a register fault between a
 * sum's read of a value and the instruction that consumes the same register. */
int fhe_polymul_checked(fhe_ctx *ctx, uint64_t *d_c, uint64_t *d_a, uint64_t *d_b, const fhe_ntt_tables *t, const fhe_abft *a,
                        size_t n_poly, size_t limbs, size_t start_idx, uint32_t *d_flags, void *stream);
/* Test hook: one bit flip (bit `bit`) inside the next fhe_polymul_checked on this context; `idx` = word of the call's
 * [poly][limb][N] window.  point 0 / 1: a's / b's column-pass output before the middle launch (N >= 2^13, flags k = 0 / 1);
 * 2: one product value of unit idx / N inside the middle launch, after the multiply (every fused size, k = 2); 3: c between the
 * middle launch and the inverse column pass (N >= 2^13, k = 2).  One shot; point < 0 clears it.  A point that does not exist
 * for the call makes it return FHE_ERR_UNSUPPORTED without launching anything. */
int fhe_ctx_inject_fault_polymul(fhe_ctx *ctx, int point, long long idx, int bit);
/* Test hook: a soft error INSIDE a pass of the next fhe_ntt_forward_checked_phases call -- XOR bit `bit` of word `lds_word`
 * (modulo the image size) of workgroup `workgroup`'s LDS image between the pass's first two register steps; pass 0 = column
 * pass, 1 = row pass, < 0 clears it.  One shot.  (The reference injects into butterfly results, relia_ntt_sim.cpp:189-194.) */
int fhe_ctx_inject_fault_in_pass(fhe_ctx *ctx, int pass, uint32_t workgroup, uint32_t lds_word, int bit);
/* Test hook for the detector: XOR bit `bit` of word `idx` of the buffer BETWEEN the two launches of the
 * next two-pass forward/inverse transform issued on this context (one shot; idx < 0 clears it).  This is
 * the in-flight analogue of the host-side flips of reliability_test/ntt_test.cu:104-135. */
int fhe_ctx_inject_fault(fhe_ctx *ctx, long long idx, int bit);

/* ---- residue-checked element-wise products (SURVEY section 8 f3, next to the detector) -------------------------------------
 * The protections of rfhe_framewk/src/barrett_final.{py,cpp} (Intra: fold residue of a, b and the product; Range: windows on
 * the Barrett intermediates; Sum: reduced against unreduced sum) for the coefficient-wise products, which a weighted checksum
 * cannot cover cheaply.  For canonical operands (a, b < q < 2^61) every product kernel forms a quotient k and a word c with
 *     a b (+ o, the old word when accumulating) = k q + c,   0 <= c < q,
 * and the checked calls verify, per word, with 32-bit lane arithmetic independent of the 64-bit multiply that made c,
 *     r(c) + r(k) r(q) == r(a) r(b) (+ r(o))  (mod m = 2^32 - 1),   r(x) = x mod m folded from the 32-bit halves,
 * plus the window c < q (for Barrett the same compare as the pre-subtraction window; for the FP64 path also the running sum and
 * the value after the reduction).  A single-bit flip of the product, of k or of c changes one side by 2^j, never 0 mod m; for
 * the five primes dividing m (3, 5, 17, 257, 65537) a change of k by a multiple of m / q is left to the window.  A consistent
 * shift (k - d, value + d q) gives the right word and raises nothing.  Not covered: faults already in the operands, and a
 * register fault on a or b before both the product and its residue have read it.
 * Output words are those of fhe_modmul / fhe_modmul_acc / fhe_tensor_product, bit for bit, for every input (Barrett for the
 * modmul pair, the per-limb FP64 / U64 choice for the tensor product); aliasing and argument rules are theirs as well.
 * Flags (zeroed on `stream` by the call; a failing word ORs its bits in with a global atomic):
 *   modmul: d_flags[poly * limbs + l];  tensor product: d_flags[3 * l + part], part 0 / 1 / 2 = d0 / d1 / d2
 *   bit 1  residue identity failed;  bit 2  a result or a reduction intermediate out of its window;
 *   bit 4  an operand (or, accumulating, the old word) not canonical -- that word cannot be checked, it raises bit 4 alone
 *          and is still the unchecked call's word.
 * No detector object: only q mod m per limb, formed in the kernel.  Calls on different streams may run concurrently. */
int fhe_modmul_checked(fhe_ctx *ctx, uint64_t *d_c, const uint64_t *d_a, const uint64_t *d_b, const fhe_ntt_tables *t,
                       size_t n_poly, size_t limbs, size_t start_idx, uint32_t *d_flags, void *stream);
int fhe_modmul_acc_checked(fhe_ctx *ctx, uint64_t *d_c, const uint64_t *d_a, const uint64_t *d_b, const fhe_ntt_tables *t,
                           size_t n_poly, size_t limbs, size_t start_idx, uint32_t *d_flags, void *stream);
int fhe_tensor_product_checked(fhe_ctx *ctx, uint64_t *d_d0, uint64_t *d_d1, uint64_t *d_d2, const uint64_t *d_a0,
                               const uint64_t *d_a1, const uint64_t *d_b0, const uint64_t *d_b1, const fhe_ntt_tables *t,
                               size_t limbs, size_t start_idx, uint32_t *d_flags, void *stream);
/* Test hook: XOR bit `bit` once, in the next checked pointwise call on this context, at element `idx` of the call's
 * [poly][limb][N] window ([limb][N] for the tensor product, where it lands in d1, the two-term sum).  point 0: the product
 * before reduction (U64: low word of the 128-bit product; FP64: h); 1: the quotient estimate of the reduction that produces the
 * word; 2: the result word before its range check and store; 3: the running sum before its final reduction -- only for
 * fhe_modmul_acc_checked and fhe_tensor_product_checked, elsewhere the call returns FHE_ERR_UNSUPPORTED and launches nothing.
 * One shot (an unsupported or out-of-window fault is used up as well); point < 0 clears it. */
int fhe_ctx_inject_fault_pointwise(fhe_ctx *ctx, int point, long long idx, int bit);

/* ---- residue-checked base conversion --------------------------------------------------------------------------------------
 * fhe_baseconv_exact / fhe_baseconv_fast with every mixed-radix digit and every output word checked: the stage that
 * motivation/baseConv.py perturbs (one input residue, then what the conversion does to it) and rfhe_framewk/src/baseConv.{py,cpp,cu}
 * compute, protected with the fold-residue and range detectors of rfhe_framewk/src/barrett_final.{py,cpp} carried through the sums.
 * A base conversion is not linear over the coefficient index, so no NTT checksum reaches it, and one wrong digit corrupts every
 * output limb of its coefficient.  Over the integers
 *     digit j    r_j A_j - sum_{l<j} c_l D_lj = K_j p_j + c_j      0 <= c_j < p_j   (K_j signed)
 *     output o   sum_l c_l E_lo               = K_o q_o + out_o    0 <= out_o < q_o
 *     fast o     sum_j in_j C_jo              = K_o q_o + out_o    every reduced term < q_o, out_o < m q_o (the sum is not reduced)
 * and the checked calls verify each identity modulo 2^32 - 1 with 32-bit lane arithmetic independent of the 64-bit multiplies
 * that made the word (the residue of K is carried, K itself can pass 64 bits), plus the windows on the right.
 * Words: d_out is fhe_baseconv_exact's / fhe_baseconv_fast's, bit for bit, for every input including words >= p_j, on both kinds
 * of plan (all moduli below 2^50, or not) and for every m, k from 1 to 64; canonical digits and outputs are unique, and the
 * checked kernels form them as Shoup products on every plan.  Argument rules, FHE_ERR_UNSUPPORTED of the fast form on a plan
 * whose unreduced sum would pass 64 bits, and the limits are the unchecked calls'.
 * Flags (zeroed on `stream` by the call; a failing coefficient ORs its bits in with a global atomic):
 *   exact: d_flags[j], j < m: the digit recurrence of input limb j;  d_flags[m + o]: output limb o.   fast: d_flags[o].
 *   bit 1  residue identity failed;  bit 2  a digit, word or reduced term out of its window;
 *   bit 4  (exact only) input word >= p_j on digit unit j: folded, not checked, raised alone; the word is still the unchecked
 *          call's.  The fast form takes any 64-bit word (its Shoup quotient fits 64 bits) and never raises bit 4.
 * Localisation: a fault raises the flag of the unit it hit and no other.  A wrong digit changes the later digits and all outputs
 * consistently, so their units stay clear (the rule of the per-phase NTT flags).
 * Not covered: faults already in the input, a register fault on a digit between its check and a later use, faults in the plan's
 * constant tables.  No detector object and no scratch: calls on different streams may run concurrently. */
int fhe_baseconv_exact_checked(fhe_ctx *ctx, uint64_t *d_out, const uint64_t *d_in, const fhe_baseconv *p, size_t N,
                               uint32_t *d_flags /* [m + k] */, void *stream);
int fhe_baseconv_fast_checked(fhe_ctx *ctx, uint64_t *d_out, const uint64_t *d_in, const fhe_baseconv *p, size_t N,
                              uint32_t *d_flags /* [k] */, void *stream);
/* Test hook: XOR bit `bit` once, in the next checked base conversion on this context, in coefficient `coeff` of unit `unit` (index
 * into that call's flags array).  point 0: low word of the 128-bit product of the unit's first term; 1: the Shoup quotient of the
 * reduction that completes the digit / word (its last term; fast form: the first term's); 2: the digit / word before its window
 * check and every later use; 3: the running sum with its last term folded in, before the conditional +- q that closes it (fast
 * form: the sum of all terms but the last) -- needs two terms: on digit 0, or on any output of a one-limb base, the call returns
 * FHE_ERR_UNSUPPORTED; a unit or coefficient outside the call returns FHE_ERR_INVALID.  Either way nothing is launched.  Where
 * the outputs are sliced over workgroups, every workgroup sees the same wrong digit.  One shot (a refused call uses it up as
 * well); point < 0 clears it. */
int fhe_ctx_inject_fault_baseconv(fhe_ctx *ctx, int point, int unit, long long coeff, int bit);

/* ---- stage-by-stage checked key switch, relinearisation and rotation -------------------------------------
 * fhe_keyswitch_apply / fhe_relinearize / fhe_rotate with every one of the eight stages of the hybrid key switch checked and one
 * uint32 flag word per (stage, unit).  d_out0 / d_out1 are the unchecked calls' words, bit for bit: every stage yields canonical
 * residues and those are unique.  d_add0 / d_add1 (optional, [L][N]) are added to the two output parts as the unchecked core does
 * (a relinearisation passes d0 and d1, a rotation sigma(c0)).  `a` must be an fhe_abft made for the plan's own table set
 * (FHE_ERR_INVALID otherwise); it is only read.  The partial sums of the transforms' checks live in the plan (allocated at the plan's
 * first checked call): one checked call at a time per plan, as for the unchecked calls.
 * Flags: fhe_keyswitch_checked_layout gives out[s] = offset of stage s (s < 8), out[8] = total words, out[9] = 0 (reserved).  The
 * call clears them on `stream`; M = L + K:
 *   stage 0  opening INTT of the L input limbs                 ABFT sums differ: 1                                   [L]
 *   stage 1  digit extension, an exact conversion per digit    bits 1 / 2 / 4 of fhe_baseconv_exact_checked          [dnum][M]
 *            entry (d, j): the mixed-radix digit unit of limb j when j belongs to digit d, the output unit of limb j otherwise
 *   stage 2  forward transform of the extended limbs           ABFT: 1                                               [dnum][M]
 *            (the digit's own limbs are not transformed: their entries stay 0)
 *   stage 3  inner product with both key halves                1 residue identity, 2 window, 4 operand >= q          [2][M]
 *   stage 4  INTT of the K special limbs of both halves        ABFT: 1                                               [2][K]
 *   stage 5  mod-down conversion P -> Q of both halves         as stage 1                                            [2][K + L]
 *            per half K digit units, then L output units
 *   stage 6  forward transform of the converted limbs          ABFT: 1                                               [2][L]
 *   stage 7  tail (acc - X) P^-1 (+ addend)                    1 / 2 / 4 as stage 3 (4: operand or addend >= q_j)    [2][L]
 * One-limb digits (dnum = L) and K = 1 make their conversion stage a conversion from one limb, x mod q_j.  There is no mixed-radix
 * recurrence and no sum to check; what runs is the checked conversion with m = 1, one product with the constant 1 per digit and per
 * output.  Its flags stay 0 on every clean run; the test hook's points 0-2 exist there and raise their unit's flag like anywhere else
 * (point 3, the running sum, does not exist: FHE_ERR_UNSUPPORTED).
 * Localisation: a fault at stage s, unit u raises the flag of (s, u) and no other flag of the call; every later stage is consistent
 * with the input it was handed.  Bit 4 marks words that could not be checked (only caller-supplied words can be non-canonical: the
 * digits' own limbs of d_c, the key, the addends); their output words are still the unchecked call's.
 * Not covered: faults already in the inputs (the sealed calls at the end of this header verify them at rest, these calls still do
 * not); a word corrupted in memory between one stage's store and the next stage's load (each check starts from the registers its
 * stage loaded); the Galois permutation of the checked rotation; operands raising bit 4.
 * Scope: a sharded plan returns FHE_ERR_INVALID; a plan with a plain modulus (BGV) FHE_ERR_UNSUPPORTED; a context with ntt_mode = 1,
 * ntt_resident or ntt_packed set, or N < 2^5, FHE_ERR_UNSUPPORTED.  The rescale and the homomorphic multiply have checked forms of
 * their own below, hoisted rotations, the Galois permutation and the BSGS product further down; BGV plans (plain modulus) have
 * the fhe_bgv_*_checked calls at the end of this header.  What remains without a checked form: sharded plans, the BGV forms of the
 * hoisted rotations and of the BSGS product, and the permutation inside fhe_rotate_checked.  A caller who wants that last one
 * checked composes it: fhe_automorphism_ntt_checked on c1 and on c0, then
 * fhe_keyswitch_apply_checked(sigma(c1), galois key, d_add0 = sigma(c0)). */
int fhe_keyswitch_checked_layout(const fhe_keyswitch *p, int out[10]);
int fhe_keyswitch_apply_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c,
                                const uint64_t *d_evk, const uint64_t *d_add0 /* optional */, const uint64_t *d_add1 /* optional */,
                                const fhe_abft *a, uint32_t *d_flags, void *stream);
int fhe_relinearize_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_d0,
                            const uint64_t *d_d1, const uint64_t *d_d2, const uint64_t *d_relin_key, const fhe_abft *a,
                            uint32_t *d_flags, void *stream);
/* sigma is applied to both parts by a launch of its own (unchecked), then sigma(c1) is key-switched with sigma(c0) as addend */
int fhe_rotate_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1,
                       uint32_t galois_elt, const uint64_t *d_galois_key, const fhe_abft *a, uint32_t *d_flags, void *stream);
/* Test hook: one bit flip of a value in flight in the next checked key switch / relinearisation / rotation on this context; `unit`
 * indexes the stage's flags (so a flip at (stage, unit) is expected to raise exactly that word).  One shot: the next checked call
 * takes it whatever its outcome; stage < 0 clears it.
 *   stages 0, 2, 4, 6: word `coeff` of the unit is flipped between the stage's two launches (`point` ignored).  Only two-launch
 *     sizes have that point: at N < 2^13 the checked call returns FHE_ERR_UNSUPPORTED, launches nothing and leaves nothing armed.
 *     A stage-2 unit that is one of its digit's own limbs returns FHE_ERR_INVALID.
 *   stages 1, 5: point / coeff as in the base conversion's hook above; the unit's position in its conversion decides which points exist
 *     (point 3 needs two terms: FHE_ERR_UNSUPPORTED on a digit's first limb and on every unit of a one-limb conversion).
 *   stages 3, 7: point 0 the first term's product before reduction (stage 7: the low word of (x - y) P^-1), 1 the quotient estimate
 *     of the reduction that produces the word, 2 the word before its window check, 3 the running sum before its final reduction
 *     (stage 7: before the conditional subtraction after the addend -- FHE_ERR_UNSUPPORTED on a half without addend);
 *     unit = half * M + row (stage 3), half * L + row (stage 7).
 * A unit or coefficient outside the call returns FHE_ERR_INVALID from the checked call. */
int fhe_ctx_inject_fault_keyswitch(fhe_ctx *ctx, int stage, int point, int unit, long long coeff, int bit);

/* ---- stage-by-stage checked rescale and homomorphic multiply ------------------------------------------------
 * fhe_rescale with every stage checked and one uint32 flag word per (stage, unit).  Argument, shape and overlap rules are
 * fhe_rescale's: d_in = [n_parts][L][N], d_out = [n_parts][L-1][N], out of place, n_parts 1 to 3.  The output words are
 * fhe_rescale's bit for bit, floor rounding included, whichever route the unchecked call took: every stage yields canonical
 * residues and those are unique.  `a` as for the checked key switch; the partial sums live in the plan.
 * Flags: fhe_rescale_checked_layout gives out[s] = offset of stage s (s < 4), out[4] = total = n_parts (1 + 3 R), out[5] = 0
 * (reserved); R = L - 1.  The call clears them on `stream`:
 *   stage 0  INTT of each part's last limb (into the plan)     ABFT sums differ: 1                                   [n_parts]
 *   stage 1  delta_j = x mod q_j for every remaining prime     1: x = k q_j + delta_j fails modulo 2^32 - 1;         [n_parts][R]
 *                                                              2: delta_j >= q_j, or the quotient estimate above x / q_j's bound;
 *                                                              4: x >= q_last -- not checkable, raised alone, the word is
 *                                                                 still x mod q_j
 *   stage 2  forward transform of the residues                 ABFT: 1                                               [n_parts][R]
 *   stage 3  (c - delta) q_last^-1                             bits 1 / 2 / 4 as stage 7 of the checked key switch   [n_parts][R]
 * Localisation as for the checked key switch: a fault at (stage, unit) raises that word and no other; later stages are consistent
 * with what they were handed.  Not covered: faults already in the input (see fhe_hmult_sealed); a word corrupted in memory between one stage's store
 * and the next stage's load; operands raising bit 4.
 * Scope: the checked key switch's -- a sharded plan FHE_ERR_INVALID; a plan with a plain modulus (BGV) FHE_ERR_UNSUPPORTED (its
 * forms are fhe_bgv_mod_switch_checked / fhe_bgv_hmult_checked); ntt_mode = 1, ntt_resident, ntt_packed, a single-pass hook or
 * N < 2^5 FHE_ERR_UNSUPPORTED; L < 2 FHE_ERR_INVALID; a detector made for another table set than the plan's FHE_ERR_INVALID. */
int fhe_rescale_checked_layout(const fhe_keyswitch *p, size_t n_parts, int out[6]);
int fhe_rescale_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out, const uint64_t *d_in, size_t n_parts, const fhe_abft *a,
                        uint32_t *d_flags, void *stream);
/* Test hook: one bit flip of a value in flight in the next fhe_rescale_checked, or in the rescale step of the next
 * fhe_hmult_checked that rescales, on this context; `unit` indexes the stage's flags.  One shot; stage < 0 clears it.
 *   stages 0, 2: word `coeff` of the unit is flipped between the transform's two launches (`point` ignored).  N >= 2^13 only: below
 *     that the checked call returns FHE_ERR_UNSUPPORTED, launches nothing and leaves nothing armed.
 *   stage 1: point 0 the product that forms the quotient estimate (high word of x times the high word of floor(2^128 / q_j)), 1
 *     the quotient estimate, 2 the word before its window check.  Point 3 does not exist (no running sum): FHE_ERR_UNSUPPORTED.
 *   stage 3: the points of stage 7 of the checked key switch; point 3 is FHE_ERR_UNSUPPORTED, the rescale has no addend.
 * A unit or coefficient outside the call returns FHE_ERR_INVALID from the checked call. */
int fhe_ctx_inject_fault_rescale(fhe_ctx *ctx, int stage, int point, int unit, long long coeff, int bit);

/* fhe_hmult with every step checked: fhe_tensor_product_checked into the plan, the checked relinearisation, and (rescale != 0)
 * the checked rescale of the two parts.  The output words are fhe_hmult's bit for bit, whether or not the unchecked call fused
 * the mod-down with the rescale; aliasing rules are fhe_hmult's (an output may reuse an operand's buffer, d_out0 != d_out1).
 * Flags, one buffer of out[3] words which the call clears on `stream` (fhe_hmult_checked_layout):
 *   out[0] = 0   the tensor block [3 L], word 3 l + part, bits of fhe_tensor_product_checked
 *   out[1]       the key-switch block, laid out as fhe_keyswitch_checked_layout
 *   out[2]       the rescale block, laid out as fhe_rescale_checked_layout with n_parts = 2 (= out[3] when rescale == 0)
 *   out[3]       total
 * The one-shot hooks fhe_ctx_inject_fault_pointwise, fhe_ctx_inject_fault_keyswitch and fhe_ctx_inject_fault_rescale each fire
 * in their own step.  All three are checked against the call before its first launch: a refused hook launches nothing and leaves
 * the flag buffer and the outputs untouched.  A status returned by any step ends the call there.  Scope and statuses as above. */
int fhe_hmult_checked_layout(const fhe_keyswitch *p, int rescale, int out[4]);
int fhe_hmult_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_a0, const uint64_t *d_a1,
                      const uint64_t *d_b0, const uint64_t *d_b1, const uint64_t *d_relin_key, int rescale, const fhe_abft *a,
                      uint32_t *d_flags, void *stream);

/* ---- checked Galois permutation and checked hoisted rotations ----------------------------------------------------
 * fhe_automorphism_ntt with one check per unit (a row of N words): d_dst[u][j] = d_src[u][pi_k(j)], pi_k the slot map of
 * fhe_automorphism_ntt.  A permutation computes nothing, so the check is a position-weighted sum per unit modulo m = 2^32 - 1,
 * r(x) = x mod m, w(j) = j + 1:
 *     S_out = sum_j w(j) r(word stored at j)          from the register about to be stored and the destination index
 *     S_in  = sum_i w(pi_kinv(i)) r(d_src[i])         from a second, linear read of d_src; kinv = k^-1 mod 2N, computed on the host
 * pi_kinv is the inverse permutation, so the sums agree on a clean run; the two sides share neither the gathered register nor the
 * index computation.  d_flags[u] = 1 where they differ (every word is written by the call, on `stream`).
 * Coverage: every single-bit flip of a moved word (it shifts S_out by +-w 2^b, never 0 modulo m); a wrong source index that fetches
 * x' for x unless w(j) (r(x') - r(x)) = 0 modulo m -- on random words with probability at most gcd(w(j), m) / m <= N / m.  Not
 * covered: a wrong galois_elt handed in by the caller, faults already in d_src, a word corrupted in memory after its store.
 * Words and argument rules are fhe_automorphism_ntt's: d_dst != d_src, odd element, n_units == 0 is a no-op.  The sums live in the
 * context (allocated at first use, grown on demand): one checked permutation at a time per context. */
int fhe_automorphism_ntt_checked(fhe_ctx *ctx, uint64_t *d_dst, const uint64_t *d_src, int log_n, uint32_t galois_elt, size_t n_units,
                                 uint32_t *d_flags /* [n_units] */, void *stream);
/* Test hook: one bit flip in the next fhe_automorphism_ntt_checked on this context, at word `coeff` of unit `unit` of the
 * destination.  point 0: XOR bit `bit` (0-63) into the gathered word before it is stored and summed; point 1: XOR bit `bit`
 * (< log_n) into the gather's source index.  A unit or coefficient outside the call, or point 1 with bit >= log_n, returns
 * FHE_ERR_INVALID from the checked call, which launches nothing.  One shot (a refused call uses it up); point < 0 clears it. */
int fhe_ctx_inject_fault_galois(fhe_ctx *ctx, int point, int unit, long long coeff, int bit);

/* fhe_rotate_hoisted with every stage checked, the Galois permutation included.  sigma is a ring automorphism and the prepared
 * keys are in the un-rotated frame, so the launch list is: stages 0, 1, 2 of the checked key switch ONCE on the un-rotated d_c1;
 * then per rotation r stage 3 (inner product of the shared digits with d_prepared_keys[r]), stage 8 (the checked permutation of the
 * 2 M rows of the sums and of the L rows of d_c0) and stages 4-7 on the rotated sums with sigma(c0) as the first part's addend.  All
 * on `stream`; no side stream, no fusion.  Every d_out0[r] / d_out1[r] is fhe_rotate_hoisted's word, bit for bit, whichever
 * route the unchecked call took (fused, grouped, two streams): canonical residues are unique.
 * Flags (cleared by the call on `stream`), fhe_rotate_hoisted_checked_layout with M = L + K:
 *   out[0..2]  offsets of stages 0-2 in the shared block, laid out as in fhe_keyswitch_checked_layout
 *   out[3..8]  offsets inside one rotation's block, in execution order: stage 3 [2][M], stage 8 [2 M + L] (unit half * M + row for
 *              the sums, then 2 M + l for row l of c0), stages 4 [2][K], 5 [2][K + L], 6 [2][L], 7 [2][L]
 *   out[9]     words of the shared block, L + 2 dnum M;  out[10]  words of one rotation's block;  out[11]  total
 * Rotation r's block starts at out[9] + r out[10].  Flag bits per stage as for the checked key switch; stage 8 holds 0 / 1.
 * Localisation: a fault in a shared stage raises its own word and changes every rotation's output; a fault in rotation r raises
 * its word in block r and leaves the other rotations' words and flags alone.
 * Scope and statuses are the checked key switch's; argument rules are fhe_rotate_hoisted's (odd elements, out of place, distinct
 * parts); n_rot == 0 returns FHE_OK and launches nothing.  The rotated sums use the plan's second set of sums (allocated at the
 * first call that needs it).  Still without a checked form: sharded plans, hoisted rotations on BGV plans. */
int fhe_rotate_hoisted_checked_layout(const fhe_keyswitch *p, size_t n_rot, int out[12]);
int fhe_rotate_hoisted_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *const *d_out0, uint64_t *const *d_out1, const uint64_t *d_c0,
                               const uint64_t *d_c1, const uint32_t *galois_elts, const uint64_t *const *d_prepared_keys, size_t n_rot,
                               const fhe_abft *a, uint32_t *d_flags, void *stream);
/* Test hook of fhe_rotate_hoisted_checked, one shot: the next such call takes it whatever its outcome; stage < 0 clears it.  The call
 * neither takes nor honours the other hooks.  Stages 0-7, their points, units and FHE_ERR_UNSUPPORTED cases are those of
 * fhe_ctx_inject_fault_keyswitch (stage 7: the first half has an addend, the second has none); stage 8 takes the points of
 * fhe_ctx_inject_fault_galois with unit indexing the rotation's [2 M + L] words.  `rot` is ignored for stages 0-2 and must be below
 * n_rot for stages 3-8 (FHE_ERR_INVALID from the checked call otherwise). */
int fhe_ctx_inject_fault_rotate_hoisted(fhe_ctx *ctx, int rot, int stage, int point, int unit, long long coeff, int bit);

/* ---- checked modular add and checked BSGS matrix-vector product --------------------------------------------------
 * fhe_modadd with every word checked: c = a + b - e q with e in {0, 1}, both operands reduced first as k_modadd reduces them.  Per
 * word, with the 32-bit lane arithmetic of the checked products,
 *     r(c) + e r(q) == r(a) + r(b)  (mod m = 2^32 - 1)      and the window c < q.
 * Words are fhe_modadd's bit for bit for every input; argument and aliasing rules are fhe_modadd's (in place allowed).  Flags:
 * d_flags[poly * limbs + l], cleared by the call on `stream`; bit 1 identity, bit 2 window, bit 4 an operand >= q -- folded as
 * fhe_modadd folds it, not checked, raised alone.  fhe_ctx_inject_fault_pointwise is honoured with points 2 (the word before its
 * window check) and 3 (a + b before the conditional subtraction); points 0 and 1 do not exist on an add: FHE_ERR_UNSUPPORTED,
 * nothing launched.  The hook is used up either way. */
int fhe_modadd_checked(fhe_ctx *ctx, uint64_t *d_c, const uint64_t *d_a, const uint64_t *d_b, const fhe_ntt_tables *t, size_t n_poly,
                       size_t limbs, size_t start_idx, uint32_t *d_flags, void *stream);

/* fhe_bsgs_matvec with every stage checked.  The launch list, all on `stream`, no side stream and no fusion:
 *   baby block (n1 > 1)  the launches of fhe_rotate_hoisted_checked for the n1 - 1 baby elements, into the plan's BSGS scratch
 *   per giant step g     inner sum  s_h = sum_b diag[g][b] sigma_b(x)_h of both parts h: per word and part
 *                        r(c) + r(K) r(q) == sum_b r(d_b) r(y_b) (mod 2^32 - 1) and the windows of stage 3 of the checked key switch
 *                        (the running sums are folded after every eighth term, as the unchecked kernel folds them);
 *                        written straight into the outputs for g = 0
 *     g >= 1             the checked Galois permutation of the 2 L rows of the inner sum, rows of part 0 first;
 *                        the checked add t0 = out0 + sigma(s0);
 *                        the checked key switch of sigma(s1) with the giant key and the addends (t0, out1), writing (out0, out1)
 * The running result rides on the addends of the switch's tail, so a giant step needs one add launch, not two.  Every stage yields
 * canonical residues, so d_out0 / d_out1 are fhe_bsgs_matvec's words bit for bit although the unchecked call adds in another order
 * and takes sigma on loads.
 * Flags, one buffer of out[7] words which the call clears on `stream` (fhe_bsgs_matvec_checked_layout):
 *   out[0] = 0  the baby block, laid out as fhe_rotate_hoisted_checked_layout(n1 - 1); out[1] words, 0 when n1 == 1
 *   out[1]      start of giant block 0;  out[2]  words of one giant block; block g starts at out[1] + g out[2]
 *   out[3..6]   offsets inside a giant block: inner sum [2][L] (part * L + l; bits 1 / 2 / 4 as stage 3 of the checked key switch,
 *               4: a diagonal word >= q on both parts, a ciphertext word >= q on its part), permutation [2 L] (0 / 1),
 *               accumulate [L] (bits of fhe_modadd_checked), key switch (fhe_keyswitch_checked_layout).  For g = 0 only the
 *               inner sum runs: the other words of block 0 stay 0.
 *   out[7]      total
 * The layout call returns FHE_ERR_INVALID for n1 or n2 outside 1 .. 4096 and for a total above INT_MAX.
 * Localisation: a fault raises the word of the (block, stage, unit) it hit and no other; a baby-block fault changes the output and
 * raises only its own word.  Not covered: faults already in the inputs, the diagonals or the keys; a word corrupted in memory
 * between one stage's store and the next stage's load; operands raising bit 4.
 * Scope and statuses are the checked key switch's (sharded plan FHE_ERR_INVALID, BGV plan FHE_ERR_UNSUPPORTED, N < 2^5
 * FHE_ERR_UNSUPPORTED, ...); argument rules are fhe_bsgs_matvec's (out of place, distinct parts, n1, n2 from 1 to 4096).  The call
 * uses the plan's BSGS scratch, both sets of sums, the rotation buffer and the check sums: one call at a time per plan.
 * Test hooks: the call takes fhe_ctx_inject_fault_rotate_hoisted (fires in the baby block), fhe_ctx_inject_fault_galois and
 * fhe_ctx_inject_fault_keyswitch (both fire in giant step g = 1, the key switch there has addends on both halves) and
 * fhe_ctx_inject_fault_bsgs at entry, whatever its outcome, and validates them before the first launch; an armed hook whose step
 * the call does not have (n1 == 1, n2 == 1) returns FHE_ERR_INVALID. */
int fhe_bsgs_matvec_checked_layout(const fhe_keyswitch *p, size_t n1, size_t n2, int out[8]);
int fhe_bsgs_matvec_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1,
                            const uint64_t *d_diags, size_t n1, size_t n2, const uint32_t *baby_elts,
                            const uint64_t *const *d_baby_keys_prepared, const uint32_t *giant_elts, const uint64_t *const *d_giant_keys,
                            const fhe_abft *a, uint32_t *d_flags, void *stream);
/* Test hook of the two stages fhe_bsgs_matvec_checked adds, one shot; stage < 0 clears it.  `g` is the giant step.
 *   stage 0  the inner sum: unit = part * L + l, points 0-3 as stage 3 of fhe_ctx_inject_fault_keyswitch (0 the first term's product,
 *            1 the final reduction's quotient estimate, 2 the word before its window check, 3 the running sum before its final
 *            reduction)
 *   stage 1  the accumulate: unit = l, point 2 the word before its window check, 3 the sum before the conditional subtraction;
 *            points 0 and 1 return FHE_ERR_UNSUPPORTED from the checked call
 * A g, unit or coefficient outside the call, and stage 1 with g = 0, return FHE_ERR_INVALID from the checked call.  A refused call
 * launches nothing and uses the hook up. */
int fhe_ctx_inject_fault_bsgs(fhe_ctx *ctx, int g, int stage, int point, int unit, long long coeff, int bit);

/* ---- checked scalar multiply and the BGV forms of the checked key switch, mod switch and multiply -----------------
 * fhe_scalar_affine with every word checked: c = a s_l + o_l mod q_l, one scalar pair per limb.  Per word, for canonical a, s, o,
 *     a s (+ o) = k q + c,   0 <= c < q,      checked as   r(c) + r(k) r(q) == r(a) r(s) (+ r(o))  (mod m = 2^32 - 1)
 * with the 32-bit lane arithmetic of the checked products, plus two windows: c < q, and k within 2^24 of the FP64 estimate
 * a s / q.  The second one is what sees a quotient moved so far that the 64-bit remainder wraps by a multiple of m words and
 * lands in [0, q) again (2^46 (2^50 - 2^18 + 1) = m 2^64 + 2^46): a product's quotient is as large as a, so no bound taken from
 * the operand's size separates the two.  A flag is raised exactly when the stored word differs from the clean one; an estimate one
 * or two too low, which the conditional subtractions absorb, gives the right word and raises nothing.
 * Words are fhe_scalar_affine's bit for bit for every input; argument rules are its own (mul == NULL: 1, add == NULL: 0, scalars
 * reduced by the call, limbs <= 64 else FHE_ERR_UNSUPPORTED with nothing launched and the flags untouched, d_c may alias d_a).
 * Flags: d_flags[poly * limbs + l], cleared by the call on `stream`; bit 1 identity, bit 2 a window, bit 4 the word a >= q --
 * multiplied as fhe_scalar_affine multiplies it, not checked, raised alone.  fhe_ctx_inject_fault_pointwise is honoured: point 0 the
 * low word of the 128-bit product, 1 the Barrett quotient estimate, 2 the word before its window check, 3 the sum a s mod q + o
 * before the conditional subtraction -- only with an addend, FHE_ERR_UNSUPPORTED and nothing launched without one.  The hook is
 * used up either way.  Not covered: faults already in d_a, a register fault on a word before the product, its residue and the
 * estimate have all read it, faults in the limb constants or the scalars. */
int fhe_scalar_affine_checked(fhe_ctx *ctx, uint64_t *d_c, const uint64_t *d_a, const uint64_t *mul, const uint64_t *add,
                              const fhe_ntt_tables *t, size_t n_poly, size_t limbs, size_t start_idx,
                              uint32_t *d_flags /* [n_poly][limbs] */, void *stream);

/* The checked key switch, relinearisation and rotation on a plan WITH a plain modulus t (fhe_keyswitch_set_plain_modulus): the
 * scheme of reliability_test/dotprod_test.cu:113-148.  A BGV mod-down removes t [acc t^-1]_P instead of [acc]_P, so the launch list
 * is stages 0-7 of the checked key switch plus two word-wise scalar stages, both in place, both the kernel of
 * fhe_scalar_affine_checked:
 *   stage 9   special limbs of both halves of the sums times t^-1 mod p_k (coefficient form)     between stages 4 and 5   [2][K]
 *   stage 10  converted limbs of both halves times t mod q_j (coefficient form)                  between stages 5 and 6   [2][L]
 * (8 stays the hoisted rotations' permutation number and is not used here.)  Signatures, argument rules and d_add0 / d_add1 are
 * those of fhe_keyswitch_apply_checked / fhe_relinearize_checked / fhe_rotate_checked; fhe_bgv_rotate_checked applies sigma
 * unchecked, as fhe_rotate_checked does.  d_out0 / d_out1 are the words of fhe_keyswitch_apply / fhe_relinearize / fhe_rotate on
 * the same plan, bit for bit, whichever route the unchecked call took (t riding on the fused tail, or a launch of its own).
 * Flags: fhe_bgv_keyswitch_checked_layout gives out[0..7] = the offsets of fhe_keyswitch_checked_layout, out[8] = offset of stage 9
 * (the CKKS-form total), out[9] = offset of stage 10, out[10] = total, out[11] = 0 (reserved).  Stages 9 and 10: unit = half * K + k
 * / half * L + j; bit 1 identity, 2 window, 4 operand >= q -- never raised on a clean run, both inputs are stage outputs.
 * Localisation: as for the checked key switch, a fault at (stage, unit) raises that word and no other.
 * Not covered: what the checked key switch does not cover (inputs at rest: fhe_hmult_sealed / fhe_rotate_sealed); faults in the plan's
 * scalars t^-1 mod p_k, t mod q_j.
 * Scope: a plan WITHOUT a plain modulus returns FHE_ERR_INVALID (use the calls above); otherwise the checked key switch's -- a
 * sharded plan FHE_ERR_INVALID, ntt_mode = 1, ntt_resident, ntt_packed, a single-pass hook or N < 2^5 FHE_ERR_UNSUPPORTED, a
 * detector made for another table set FHE_ERR_INVALID -- and L, K <= 64 (FHE_ERR_UNSUPPORTED).  Still without a checked form:
 * the BGV forms of fhe_rotate_hoisted_checked and fhe_bsgs_matvec_checked, sharded plans. */
int fhe_bgv_keyswitch_checked_layout(const fhe_keyswitch *p, int out[12]);
int fhe_bgv_keyswitch_apply_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c,
                                    const uint64_t *d_evk, const uint64_t *d_add0 /* optional */, const uint64_t *d_add1 /* optional */,
                                    const fhe_abft *a, uint32_t *d_flags, void *stream);
int fhe_bgv_relinearize_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_d0,
                                const uint64_t *d_d1, const uint64_t *d_d2, const uint64_t *d_relin_key, const fhe_abft *a,
                                uint32_t *d_flags, void *stream);
int fhe_bgv_rotate_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0,
                           const uint64_t *d_c1, uint32_t galois_elt, const uint64_t *d_galois_key, const fhe_abft *a,
                           uint32_t *d_flags, void *stream);
/* mod_switch_to_next on a BGV plan (fhe_rescale's words there, bit for bit): the checked rescale's stages 0-3 plus
 *   stage 4  each part's last limb in coefficient form times t^-1 mod q_last                      between stages 0 and 1   [n_parts]
 *   stage 5  the residues times t mod q_j                                                         between stages 1 and 2   [n_parts][R]
 * so that the removed part is t [c t^-1]_{q_last}.  Arguments of fhe_rescale_checked.  fhe_bgv_mod_switch_checked_layout gives
 * out[0..3] as fhe_rescale_checked_layout, out[4] / out[5] = offsets of stages 4 / 5, out[6] = total, out[7] = 0.  Flag bits of
 * stages 4 and 5 as stages 9 and 10 above; scope as above, and L < 2 FHE_ERR_INVALID. */
int fhe_bgv_mod_switch_checked_layout(const fhe_keyswitch *p, size_t n_parts, int out[8]);
int fhe_bgv_mod_switch_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out, const uint64_t *d_in, size_t n_parts, const fhe_abft *a,
                               uint32_t *d_flags, void *stream);
/* fhe_hmult on a BGV plan with every step checked -- multiply -> relinearize_inplace -> mod_switch_to_next_inplace as the
 * reference's dot product runs them: fhe_tensor_product_checked, the BGV checked relinearisation, and (rescale != 0) the BGV
 * checked mod switch of both parts.  Arguments and aliasing rules of fhe_hmult_checked; the words are fhe_hmult's on the same plan.
 * Blocks as in fhe_hmult_checked_layout with the two BGV layouts: out[0] = 0 tensor [3 L], out[1] the key-switch block
 * (fhe_bgv_keyswitch_checked_layout), out[2] the mod-switch block (fhe_bgv_mod_switch_checked_layout, n_parts = 2; = out[3] when
 * rescale == 0), out[3] total. */
int fhe_bgv_hmult_checked_layout(const fhe_keyswitch *p, int rescale, int out[4]);
int fhe_bgv_hmult_checked(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_a0, const uint64_t *d_a1,
                          const uint64_t *d_b0, const uint64_t *d_b1, const uint64_t *d_relin_key, int rescale, const fhe_abft *a,
                          uint32_t *d_flags, void *stream);
/* Test hooks of the BGV calls, one shot each, with records of their own: the BGV calls take only these (fhe_bgv_hmult_checked
 * also fhe_ctx_inject_fault_pointwise for its tensor step) and neither take nor honour fhe_ctx_inject_fault_keyswitch / _rescale;
 * the calls above do not take these.  A hook is checked against the call before its first launch; a refused call launches
 * nothing and uses the hook up.  stage < 0 clears.
 *   _bgv_keyswitch: stages 0-7 as fhe_ctx_inject_fault_keyswitch; stages 9 and 10: point 0 the low word of the product, 1 the
 *     quotient estimate, 2 the word before its window check; point 3 returns FHE_ERR_UNSUPPORTED from the checked call (no addend,
 *     no sum).  Stage 8 is refused by the setter: FHE_ERR_INVALID.
 *   _bgv_mod_switch: stages 0-3 as fhe_ctx_inject_fault_rescale; stages 4 and 5 as stages 9 and 10. */
int fhe_ctx_inject_fault_bgv_keyswitch(fhe_ctx *ctx, int stage, int point, int unit, long long coeff, int bit);
int fhe_ctx_inject_fault_bgv_mod_switch(fhe_ctx *ctx, int stage, int point, int unit, long long coeff, int bit);

/* ---- seals: operands protected at rest, sealed multiply and rotation ---------------------------------------------
 * Every checked call above ends its coverage note with "faults already in the inputs": a word that is wrong in memory before the
 * call loads it -- the bit flips of reliability_test/dotprod_test.cu:31-61 in the limbs of an encrypted operand, a word that rots
 * between one call's store and the next call's load, a flipped word of a switching key -- is a consistent input to every stage and
 * raises nothing.  A seal is an integrity record that travels with a ciphertext or key between calls: per row of N words of limb l,
 * with p = 2^61 - 1 (prime),
 *     S0 = sum_j x_j mod p,      S1 = sum_j (j + 1) x_j mod p,      and the window x_j < q_l,
 * stored as uint64_t [rows][2] = {S0, S1}, canonical in [0, p) (p itself is 0); rows in [poly][limb] order like fhe_modadd_checked.
 * Not the 2^32 - 1 fold of the checked products: that modulus is composite and 2^32 = 1 in it, so +2^b - 2^(b+32) inside one word
 * is invisible, and the reference flips several bits per symbol.  With p prime and every canonical word below q < 2^61 <= p:
 *   a change confined to one word of a row is caught with certainty (the new word is >= q: window; else 0 < |d| < p moves S0);
 *   a change confined to two words j1 != j2 is caught with certainty (d1 + d2 = 0 and (j1 - j2) d1 = 0 force d1 = 0, 0 < |j1 - j2| < p);
 *   wider corruption escapes with probability about 2^-61 per sum on random data.
 * fhe_seal writes the seals of d_words = [n_poly][limbs][N] (limb i on modulus start_idx + i) to d_seal = [n_poly * limbs][2].
 * fhe_seal_verify sweeps the same rows and ORs into d_flags[row] (uint32, cleared by the call on `stream`): bit 1 a sum differs from
 * d_seal[row], bit 2 some word >= q_l.  n_poly == 0 or limbs == 0 is a no-op; a range outside the table set FHE_ERR_INVALID; d_words
 * must be 16-byte aligned (FHE_ERR_INVALID), N >= 2.  Integer arithmetic modulo p throughout: the seal does not depend on how the
 * rows are spread over the chip, reruns give identical seals.  The chunks' partial sums live in the context (grown on demand): one
 * seal call or sealed composite at a time per context.
 * Test hook: fhe_ctx_inject_fault_seal(row, coeff, bit) flips bit `bit` of word `coeff` of row `row` of the next fhe_seal or
 * fhe_seal_verify on this context in the register, after the load and before it is summed and held against q: memory stays clean.
 * One shot, taken by that call whatever its outcome; a row or word outside the call returns FHE_ERR_INVALID from it, with nothing
 * launched; row < 0 clears.  The sealed composites below neither take nor honour it. */
int fhe_seal(fhe_ctx *ctx, uint64_t *d_seal, const uint64_t *d_words, const fhe_ntt_tables *t, size_t n_poly, size_t limbs, size_t start_idx,
             void *stream);
int fhe_seal_verify(fhe_ctx *ctx, const uint64_t *d_words, const uint64_t *d_seal, const fhe_ntt_tables *t, size_t n_poly, size_t limbs,
                    size_t start_idx, uint32_t *d_flags, void *stream);
int fhe_ctx_inject_fault_seal(fhe_ctx *ctx, int row, long long coeff, int bit);
/* The checked multiply and the checked rotation with their operands protected at rest.  One name for both schemes: on a plan with a
 * plain modulus the call runs fhe_bgv_hmult_checked / fhe_bgv_rotate_checked, otherwise fhe_hmult_checked / fhe_rotate_checked.  Order
 * of work, all on `stream`: verify every given seal, run the checked call unchanged, seal both outputs.  Arguments are the checked
 * call's, plus
 *   d_seal_in   HOST array of device pointers to the seals of a0, a1, b0, b1 (multiply) / c0, c1 (rotation), each [L][2]; an entry,
 *               or the array, may be NULL: that operand is unsealed and not verified, its flag words stay 0
 *   d_seal_key  seal of the relinearisation / Galois key, [dnum][2][L + K][2] over the plan's whole table set
 *               (fhe_seal(key, t, dnum * 2, L + K, 0)); may be NULL
 *   d_seal_out  HOST array of two device pointers, [L][2] each ([L - 1][2] after a rescale): the seals of d_out0 and d_out1 as the
 *               call stored them; an entry, or the array, may be NULL
 * Flags, one buffer which the call clears on `stream`:
 *   fhe_hmult_sealed_layout   out[0..3] the rows of a0, a1, b0, b1 ([L] each), out[4] the key's rows [dnum][2][L + K], out[5] the
 *                             checked call's own block, exactly fhe_hmult_checked_layout's / fhe_bgv_hmult_checked_layout's, out[6]
 *                             total, out[7] = 0 (reserved)
 *   fhe_rotate_sealed_layout  out[0..1] the rows of c0, c1, out[2] the key's rows, out[3] the checked call's block
 *                             (fhe_keyswitch_checked_layout / fhe_bgv_keyswitch_checked_layout), out[4] total, out[5] = 0
 * Input and key words hold the bits of fhe_seal_verify.  A raised input flag does not stop the call: the caller reads the flags
 * afterwards, as everywhere else -- the flags of the checked block and the output seals are then meaningless, the call computed on a
 * corrupted operand and sealed what came out.  The output words are fhe_hmult's / fhe_rotate's on the same plan, bit for bit.
 * Scope, statuses, aliasing rules and test hooks are the underlying checked call's; a call outside its scope returns its status
 * with nothing launched.  A status from the checked call after the verifying launches (a refused hook) leaves the input and key flags
 * written and no output seal.  Every buffer must be 16-byte aligned (FHE_ERR_INVALID).
 * Still not covered, for multiply and rotation: the verifying read and the consuming read are two loads, so a transient fault on the
 * second one alone is not seen; neither is a word corrupted between the checked call's final store and the sealing launch's load.
 * For add and subtract both gaps are closed (fhe_modadd_sealed / fhe_modsub_sealed below: the digest is taken from the register
 * about to be stored, and the operands are verified on the consumer's own load).  Sharded plans, the hoisted rotations and the
 * BSGS product have no sealed form. */
int fhe_hmult_sealed_layout(const fhe_keyswitch *p, int rescale, int out[8]);
int fhe_hmult_sealed(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_a0, const uint64_t *d_a1,
                     const uint64_t *d_b0, const uint64_t *d_b1, const uint64_t *d_relin_key, int rescale, const fhe_abft *a,
                     const uint64_t *const *d_seal_in /* [4] */, const uint64_t *d_seal_key, uint64_t *const *d_seal_out /* [2] */,
                     uint32_t *d_flags, void *stream);
int fhe_rotate_sealed_layout(const fhe_keyswitch *p, int out[6]);
int fhe_rotate_sealed(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1,
                      uint32_t galois_elt, const uint64_t *d_galois_key, const fhe_abft *a, const uint64_t *const *d_seal_in /* [2] */,
                      const uint64_t *d_seal_key, uint64_t *const *d_seal_out /* [2] */, uint32_t *d_flags, void *stream);

/* ---- repair: locate and correct one corrupted word per sealed row ------------------------------------------------
 * A raised seal flag so far left the caller nothing to do but discard the operand.  A third sum per row, the locator
 *     S2 = sum_j (j + 1)^2 x_j mod p,
 * kept beside the seal as uint64_t [rows] (canonical), makes {S0, S1, S2} a single-error-correcting code.  With the syndromes
 * D_i = (sum of the row as it is now) - (stored sum), a change d in one word j gives D0 = d, D1 = w d, D2 = w^2 d with w = j + 1:
 * w = D1 / D0 names the word and x = x' - d restores it exactly, since x < q < p.  The locator is required because two sums are not
 * safe: the same bit set in words j1, j2 with j1 + j2 even gives D1 / D0 = the midpoint's weight, and an intact word would be
 * "corrected" into a row that passes its seal.  For two changed words D1^2 - D0 D2 = -d1 d2 (w1 - w2)^2 is non-zero modulo the prime
 * p, so the consistency test D1^2 = D0 D2 fails with certainty.
 * Guarantees, per row:
 *   one corrupted word, any 64-bit pattern: restored exactly (x' = x + k p, which no sum sees, through the window);
 *   two corrupted words: never written to, with certainty;
 *   three or more corrupted words: miscorrected with probability about N / p on random data;
 *   a corrupted seal or locator word beside an intact row moves one sum: FHE_SEAL_SUSPECT; beside a corrupted row the syndromes are
 *     inconsistent: FHE_SEAL_UNCORRECTABLE.  Neither writes.  A row is examined only when fhe_seal_verify's sweep raises it, so a
 *     corrupted locator beside an intact row and seal goes unnoticed (FHE_SEAL_CLEAN) until that row is first flagged.
 * Outcomes (report word 0): */
#define FHE_SEAL_CLEAN 0         /* the row was not flagged */
#define FHE_SEAL_REPAIRED 1      /* one word corrected and confirmed by a second sweep; the flag is cleared */
#define FHE_SEAL_UNCORRECTABLE 2 /* inconsistent syndromes, index out of range, restored word >= q, window disagreement or a failed
                                    confirmation: the row is as it was found, the flag stays raised */
#define FHE_SEAL_TRANSIENT 3     /* flagged by the first sweep, but the re-read finds every sum equal and every word in its window:
                                    nothing written, the flag is cleared */
#define FHE_SEAL_SUSPECT 4       /* exactly one of the three sums differs and every word is in its window: row corruption that leaves
                                    two sums alone needs three or more words, so the stored sum is the likely casualty; the row is
                                    untouched and the flag stays raised -- the caller decides whether to reseal */
/* fhe_seal_locator writes the locators of d_words = [n_poly][limbs][N] to d_locator = [n_poly * limbs]; arguments and rules as
 * fhe_seal; it neither takes nor honours the seal hook.
 * fhe_seal_repair is fhe_seal_verify's sweep followed by the repair, asynchronous on `stream` with no host decision (usable inside a
 * stream capture once the context's scratch exists): d_words is WRITTEN where a row is repaired; d_flags[row] as fhe_seal_verify,
 * cleared again for REPAIRED and TRANSIENT rows; d_report = uint64_t [rows][4] = {outcome, index of the word, the word before, the
 * word after} (zeros beyond the outcome unless REPAIRED), 16-byte aligned.  Argument rules are fhe_seal_verify's; a null locator or
 * report is FHE_ERR_INVALID.  It takes the one-shot hook fhe_ctx_inject_fault_seal and honours it in its first sweep only: the
 * re-read then finds memory clean -- the source of FHE_SEAL_TRANSIENT. */
int fhe_seal_locator(fhe_ctx *ctx, uint64_t *d_locator, const uint64_t *d_words, const fhe_ntt_tables *t, size_t n_poly, size_t limbs,
                     size_t start_idx, void *stream);
int fhe_seal_repair(fhe_ctx *ctx, uint64_t *d_words, const uint64_t *d_seal, const uint64_t *d_locator, const fhe_ntt_tables *t, size_t n_poly,
                    size_t limbs, size_t start_idx, uint32_t *d_flags, uint64_t *d_report, void *stream);
/* fhe_hmult_sealed / fhe_rotate_sealed with every given (seal, locator) pair repaired in place instead of only verified; the same
 * body otherwise, so the operand and key pointers are not const.  d_locator_in / d_locator_key go with d_seal_in / d_seal_key, entry
 * by entry: both given or both NULL (FHE_ERR_INVALID otherwise, nothing launched).  d_locator_out: HOST array of two device pointers
 * ([L] or [L - 1] words each) for the locators of the outputs; an entry, or the array, may be NULL.  d_flags is 16-byte aligned and
 * holds the sealed call's layout followed by one report block of four uint64_t per input and key row, in the order of their flag
 * words; rows without a seal report FHE_SEAL_CLEAN:
 *   fhe_hmult_sealed_repair_layout   out[0..6] = fhe_hmult_sealed_layout's, out[7] the report block's offset in flag words (a
 *                                    multiple of 4), out[8] the total in flag words, out[9] = 0
 *   fhe_rotate_sealed_repair_layout  out[0..4] = fhe_rotate_sealed_layout's, out[5] the report block, out[6] the total, out[7] = 0
 * A row left UNCORRECTABLE or SUSPECT does not stop the call.  Not covered: faults in flight in the checked body (flags only, as
 * before), sharded plans, hoisted rotations, the BSGS product. */
int fhe_hmult_sealed_repair_layout(const fhe_keyswitch *p, int rescale, int out[10]);
int fhe_hmult_sealed_repair(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, uint64_t *d_a0, uint64_t *d_a1, uint64_t *d_b0,
                            uint64_t *d_b1, uint64_t *d_relin_key, int rescale, const fhe_abft *a, const uint64_t *const *d_seal_in /* [4] */,
                            const uint64_t *const *d_locator_in /* [4] */, const uint64_t *d_seal_key, const uint64_t *d_locator_key,
                            uint64_t *const *d_seal_out /* [2] */, uint64_t *const *d_locator_out /* [2] */, uint32_t *d_flags, void *stream);
int fhe_rotate_sealed_repair_layout(const fhe_keyswitch *p, int out[8]);
int fhe_rotate_sealed_repair(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, uint64_t *d_c0, uint64_t *d_c1, uint32_t galois_elt,
                             uint64_t *d_galois_key, const fhe_abft *a, const uint64_t *const *d_seal_in /* [2] */,
                             const uint64_t *const *d_locator_in /* [2] */, const uint64_t *d_seal_key, const uint64_t *d_locator_key,
                             uint64_t *const *d_seal_out /* [2] */, uint64_t *const *d_locator_out /* [2] */, uint32_t *d_flags, void *stream);

/* ---- seals carried through add and subtract; sealed rotate-and-sum ------------------------------------------------
 * The seal is linear and so are these two operations.  With canonical operands c_j = a_j + b_j - e_j q, e_j in {0, 1}, hence for
 * i = 0, 1, 2 and the weights w_j = j + 1
 *     S_i(c) = S_i(a) + S_i(b) - q E_i   (mod p),      E_i = sum_j w_j^i e_j,
 * and for the subtract c = a - b + e q: S_i(c) = S_i(a) - S_i(b) + q E_i.  fhe_modadd_sealed / fhe_modsub_sealed are fhe_modadd /
 * fhe_modsub (the same words for every 64-bit input, bit for bit) in one sweep that loads each operand word once, counts the wraps,
 * digests c from the register it then stores, and holds that digest against the sums predicted from the operands' seals.  Caught in
 * the same pass, on the consumer's own load: a word of a or b that differs from what was sealed, a fault in the adder, a fault in
 * the wrap count.  d_flags[row] (uint32 [n_poly * limbs], cleared by the call on `stream`): bit 1 the digest differs from the
 * prediction (or a stored sum of an operand is not canonical), bit 2 an operand word >= q_l -- such a word is reduced as fhe_modadd
 * reduces it and, where the sealed word was canonical, raises bit 1 as well.
 * d_seal_c / d_locator_c receive the PREDICTED sums, matched or not: a fault after the digest (the store, memory) is caught by the
 * next verification of c, and a raised row stays raised through every later carried operation.  On a clean run they equal fhe_seal /
 * fhe_seal_locator of c.  d_c may be d_a or d_b, d_seal_c may be d_seal_a or d_seal_b (likewise the locators), d_a may be d_b.
 * Locators are given all three or none (FHE_ERR_INVALID); a null seal is FHE_ERR_INVALID; alignment, N >= 2, the range rule and the
 * context's scratch are fhe_seal's.  Memory traffic is fhe_modadd's, 24 N bytes per row.
 * Test hook: fhe_ctx_inject_fault_seal_carry(call, point, row, coeff, bit) flips bit `bit` at word `coeff` of row `row` in the
 * call-th carry launch on this context after arming (0 = the next; fhe_modadd_sealed / fhe_modsub_sealed are one launch each, the
 * adds of fhe_rotate_sum_sealed are numbered 2 s + h), in registers: point 0 the word of a after its load, 1 the word of b, 2 c
 * before the digest and the store, 3 c after the digest and before the store (nothing is raised in that call; the next verification
 * of c raises bit 1), 4 the wrap bit as counted (`bit` is ignored).  One shot; a row or word outside the call that takes it returns
 * FHE_ERR_INVALID from that call, with nothing launched; row < 0 clears. */
int fhe_modadd_sealed(fhe_ctx *ctx, uint64_t *d_c, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_seal_c, const uint64_t *d_seal_a,
                      const uint64_t *d_seal_b, uint64_t *d_locator_c, const uint64_t *d_locator_a, const uint64_t *d_locator_b,
                      const fhe_ntt_tables *t, size_t n_poly, size_t limbs, size_t start_idx, uint32_t *d_flags, void *stream);
int fhe_modsub_sealed(fhe_ctx *ctx, uint64_t *d_c, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_seal_c, const uint64_t *d_seal_a,
                      const uint64_t *d_seal_b, uint64_t *d_locator_c, const uint64_t *d_locator_a, const uint64_t *d_locator_b,
                      const fhe_ntt_tables *t, size_t n_poly, size_t limbs, size_t start_idx, uint32_t *d_flags, void *stream);
int fhe_ctx_inject_fault_seal_carry(fhe_ctx *ctx, int call, int point, int row, long long coeff, int bit);
/* The tail of the reference's dot product (reliability_test/dotprod_test.cu:143-148: rotated = xy; rotate_inplace(rotated, step);
 * add_inplace(xy, rotated), per step) as one protected call in which every load is a verified load.  Per step s < n_steps:
 *   1. fhe_rotate_sealed from (d_c0, d_c1) into (d_tmp0, d_tmp1) with galois_elts[s] and d_galois_keys[s]: it verifies the carried
 *      seals d_seal[0..1] and the key's seal d_seal_keys[s] (the array, or an entry, may be NULL: not verified), runs the checked
 *      rotation in the plan's CKKS or BGV form and seals the rotated copy into d_seal_tmp[0..1];
 *   2. two carried adds d_c<h> += d_tmp<h>, the seals d_seal[h] updated in place.
 * d_c0, d_c1 are in/out accumulators [L][N], d_tmp0, d_tmp1 [L][N] hold the last rotated copy; galois_elts, d_galois_keys, d_seal,
 * d_seal_keys and d_seal_tmp are HOST arrays (of n_steps, n_steps, 2, n_steps and 2 entries), seals [L][2].
 * Flags: fhe_rotate_sum_sealed_layout gives out[0] the stride between the steps' blocks, out[1] the offset of the add rows inside a
 * step's block, out[2] the total, out[3] = 0; a step's block is fhe_rotate_sealed_layout's block followed by the add rows of c0 [L]
 * and of c1 [L], with the bits above.  Step s + 1 verifies on entry what step s's adds stored, and the final seals are handed back
 * for the next sealed call, so there is no closing sweep.  The words are those of the chain fhe_rotate + fhe_modadd, bit for bit.
 * A call outside the checked rotation's scope returns that call's status with nothing launched, as does an even Galois element, a
 * null key or a misaligned buffer in any step; a null seal pointer is FHE_ERR_INVALID.  The checked call's one-shot hooks fire in
 * the first step that takes them.  Not in this change: a repairing form of this composite, and sharded plans. */
int fhe_rotate_sum_sealed_layout(const fhe_keyswitch *p, int n_steps, int out[4]);
int fhe_rotate_sum_sealed(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_c0, uint64_t *d_c1, uint64_t *d_tmp0, uint64_t *d_tmp1, int n_steps,
                          const uint32_t *galois_elts, const uint64_t *const *d_galois_keys, const fhe_abft *a, uint64_t *const *d_seal /* [2] */,
                          const uint64_t *const *d_seal_keys /* [n_steps] */, uint64_t *const *d_seal_tmp /* [2] */, uint32_t *d_flags, void *stream);
/* fhe_bsgs_matvec_checked with its operands protected at rest, and the diagonals -- the largest and longest-lived operand of the
 * call -- verified on the very load that multiplies them.  CKKS plans only, the scope of fhe_bsgs_matvec_checked.  On `stream`:
 *   1. sweeps of their own (fhe_seal_verify's) over c0 and c1 against d_seal_in[0..1] ([L][2]), over every prepared baby key against
 *      d_seal_baby_keys[b] and every giant key against d_seal_giant_keys[g] ([dnum 2 (L + K)][2]; seal the PREPARED baby key, as the
 *      caller holds it);
 *   2. the baby block of fhe_bsgs_matvec_checked, unchanged;
 *   3. per giant step the inner sum of fhe_bsgs_matvec_checked -- same terms, order, folds, residue flags and fault points -- in a
 *      kernel that digests every diagonal word from the register it hands to the product, with the weight of its index in the row,
 *      and holds each row's two sums and the window word < q_l against d_seal_diags[(g n1 + b) L + l][2] (fhe_seal of d_diags with
 *      n_poly = n1 n2).  No diagonal word is read twice, and a transient fault on the consuming load is seen.  n1 > 16: a verifying
 *      sweep over the step's n1 L diagonal rows precedes the checked inner sum instead; the flags are laid out the same.  The rest
 *      of the giant step is fhe_bsgs_matvec_checked's;
 *   4. fhe_seal of both outputs into d_seal_out[0..1] ([L][2]; the array or an entry may be NULL).
 * The seal arrays are HOST arrays of device pointers; an array, or an entry, may be NULL: that operand is not verified (NULL
 * d_seal_diags: the inner sum is fhe_bsgs_matvec_checked's).  A raised input flag does not stop the call.  The words are
 * fhe_bsgs_matvec's, bit for bit.
 * Flags, cleared by the call: [c0: L][c1: L][baby keys: (n1 - 1) key rows][giant keys: (n2 - 1) key rows][diagonals: n2 n1 L]
 * [fhe_bsgs_matvec_checked's own block, exactly its layout], input words with the bits of fhe_seal_verify (1 a sum differs or a
 * stored sum is not canonical, 2 a word >= q_l).  fhe_bsgs_matvec_sealed_layout gives the six offsets in out[0..5], the total in
 * out[6], out[7] = 0; FHE_ERR_INVALID for n1 or n2 outside 1 .. 4096 and for a total above INT_MAX.
 * Every buffer (outputs, c0, c1, diagonals, keys) must be 16-byte aligned, else FHE_ERR_INVALID before any launch; otherwise the
 * statuses and argument rules are fhe_bsgs_matvec_checked's, and its hooks are taken and fire as there.
 * Test hook: fhe_ctx_inject_fault_bsgs_sealed(g, b, limb, coeff, bit), one shot, g < 0 clears; taken by the next
 * fhe_bsgs_matvec_sealed whatever its outcome.  n1 <= 16: the bit of diagonal word (g, b, limb, coeff) is flipped in the register as
 * loaded, before both the digest and the product read it -- a fault on the consuming load: the (g, b, limb) word is raised and the
 * product changes, while the residue flags stay 0.  n1 > 16: the flip lives in the verifying sweep's load only, as
 * fhe_ctx_inject_fault_seal's.  A hook outside the call (g >= n2, b >= n1, limb >= L, coeff >= N, or no diagonal seals) returns
 * FHE_ERR_INVALID with nothing launched.
 * Not covered: the baby rotations, which sit in the plan's scratch and are re-read by every giant step; the key rows are verified
 * by a sweep of their own, not on the key switch's loads; no repairing form; BGV and sharded plans. */
int fhe_bsgs_matvec_sealed_layout(const fhe_keyswitch *p, size_t n1, size_t n2, int out[8]);
int fhe_bsgs_matvec_sealed(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1,
                           const uint64_t *d_diags, size_t n1, size_t n2, const uint32_t *baby_elts,
                           const uint64_t *const *d_baby_keys_prepared, const uint32_t *giant_elts, const uint64_t *const *d_giant_keys,
                           const fhe_abft *a, const uint64_t *const *d_seal_in /* [2] */, const uint64_t *const *d_seal_baby_keys /* [n1 - 1] */,
                           const uint64_t *const *d_seal_giant_keys /* [n2 - 1] */, const uint64_t *d_seal_diags, uint64_t *const *d_seal_out /* [2] */,
                           uint32_t *d_flags, void *stream);
int fhe_ctx_inject_fault_bsgs_sealed(fhe_ctx *ctx, int g, int b, int limb, long long coeff, int bit);

/* ---- sealed tensor product: operands verified on the load that multiplies them ----------------------------------------------
 * fhe_hmult_sealed verifies a0, a1, b0, b1 in four sweeps and then multiplies from a second load of the same words: a word that is
 * wrong on that second load only passes the seal, is a consistent operand of the residue identity, and gives a wrong product with
 * no flag.  The tensor product reads each operand word exactly once, so here the seal is digested from the register that is handed
 * to the product.
 *
 * fhe_tensor_product_sealed: fhe_tensor_product_checked over rows [n_poly][limbs] (row u on table limb start_idx + u % limbs) --
 * same terms, order, arithmetic paths, residue flags and pointwise fault points -- in one kernel that digests every word of a0, a1,
 * b0, b1 from the register as loaded, with the weight of its index in the row, and a finish launch that holds each row's two sums
 * word for word against d_seal_in[0..3] ([rows][2], fhe_seal's).  d_seal_in is a HOST array of device pointers; a NULL entry, or a
 * NULL array, is not compared -- the window word < q_l is always checked.  d_seal_out: a HOST array of three device pointers
 * ([rows][2]) that receive the seals of d0, d1, d2, digested from the registers that are stored: a fault after the store is the next
 * verification's to catch.  A NULL entry is skipped; a NULL array or three NULL entries: no result is digested.  The words are
 * fhe_tensor_product's, bit for bit, also where an operand word is not canonical: such a word is flagged, not fixed.
 * Flags, cleared by the call, with R = n_poly limbs: [a0: R][a1: R][b0: R][b1: R][tensor: R x 3]; operand words with the bits of
 * fhe_seal_verify (1 the row as loaded is not the row that was sealed, or a stored sum is not canonical; 2 a word >= q_l), the
 * tensor block with the bits of fhe_tensor_product_checked, word 3 u + part.  A changed operand word raises its row and NOT the
 * tensor block: the residue identity holds on the operand as loaded.  fhe_tensor_product_sealed_layout gives the five offsets
 * {0, R, 2R, 3R, 4R} in out[0..4] and the total 7R in out[5].
 * Guarantees (seal_check.hpp): a change confined to one or two words of an operand row -- at rest, or on this call's own load --
 * is caught with certainty; wider corruption escapes with probability about 2^-61 per sum on random data.
 * An output may be exactly an operand's buffer, and a and b may be the same ciphertext.  FHE_ERR_INVALID with nothing launched
 * for a NULL argument, a limb range outside the tables, or a data buffer that is not 16-byte aligned; FHE_ERR_UNSUPPORTED for
 * log_n < 1.  The call takes the pointwise hook (fhe_ctx_inject_fault_pointwise: idx = row N + coefficient, on the d1 sum) and the
 * hook below, one shot, whatever its outcome.
 * Test hook: fhe_ctx_inject_fault_tensor_sealed(operand, row, coeff, bit), operand 0..3 = a0, a1, b0, b1, negative clears; taken by
 * the next fhe_tensor_product_sealed or fhe_hmult_sealed_fused.  The bit of that operand word is flipped in the register as loaded,
 * before window, digest and product read it; memory stays clean.  FHE_ERR_INVALID for operand > 3, a negative row or coeff, or a
 * bit outside 0..63; a row or coeff outside the call that takes it makes that call return FHE_ERR_INVALID with nothing launched.
 *
 * fhe_hmult_sealed_fused: fhe_hmult_sealed (same arguments, same flag layout: fhe_hmult_sealed_layout, same words) with the four
 * operand sweeps gone and the checked multiply's tensor step replaced by the kernel above, which writes the operands' row flags
 * where the sweeps wrote them and the residue flags where fhe_tensor_product_checked writes them.  The key is still verified by a
 * sweep; key switch, rescale and output seals are unchanged; CKKS or BGV form by the plan's plain modulus, with that form's hooks.
 * A NULL operand seal is not compared, but the window of that operand is still checked (fhe_hmult_sealed skips such an operand).
 * Not covered: the key rows, verified by a sweep and loaded again by the key switch; the plan's d0, d1, d2, which the key switch
 * re-reads; no repairing form (repair needs the sweep); sharded plans. */
int fhe_tensor_product_sealed_layout(size_t n_poly, size_t limbs, int out[6]);
int fhe_tensor_product_sealed(fhe_ctx *ctx, uint64_t *d_d0, uint64_t *d_d1, uint64_t *d_d2, const uint64_t *d_a0, const uint64_t *d_a1,
                              const uint64_t *d_b0, const uint64_t *d_b1, const fhe_ntt_tables *t, size_t n_poly, size_t limbs, size_t start_idx,
                              const uint64_t *const *d_seal_in /* [4] */, uint64_t *const *d_seal_out /* [3] */, uint32_t *d_flags, void *stream);
int fhe_ctx_inject_fault_tensor_sealed(fhe_ctx *ctx, int operand, int row, long long coeff, int bit);
int fhe_hmult_sealed_fused(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_a0, const uint64_t *d_a1,
                           const uint64_t *d_b0, const uint64_t *d_b1, const uint64_t *d_relin_key, int rescale, const fhe_abft *a,
                           const uint64_t *const *d_seal_in, const uint64_t *d_seal_key, uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream);

/* ---- sealed key-switch inner product: the switching key verified on the load that multiplies it -----------------------------
 * The sealed composites verify the key's rows in a sweep of their own and the checked key switch then loads the key a second time
 * for its inner product (stage 3): a key word that is wrong on that second load only passes the seal, is a consistent operand of
 * the residue identity, and pollutes both halves of the result with no flag.  The inner product reads each key word exactly once,
 * so here the seal is digested from the register that is handed to the product, one digest per (digit, half) of the row, and a
 * finish launch holds each key row's two sums word for word against d_seal_key ([dnum 2 M][2], fhe_seal's over the key as
 * [dnum 2][M] rows, M = L + K).  Same terms, order, arithmetic paths, residue flags and fault points as the checked stage 3.
 *
 * fhe_keyswitch_apply_sealed: fhe_keyswitch_apply_checked with stage 3 replaced by that kernel; CKKS or BGV form by the plan's
 * plain modulus, with that form's hook.  Flags, cleared by the call: [key rows: dnum 2 M, word (d 2 + h) M + j][the checked key
 * switch's own block, exactly its layout]; key words with the bits of fhe_seal_verify (1 the row as loaded is not the row that was
 * sealed, or a stored sum is not canonical; 2 a word >= q_j).  A NULL d_seal_key is not compared, but the window is still checked.
 * A changed key word raises its row and NOT the stage-3 residue flags: the identity holds on the key as loaded; the words are then
 * the product with the key as loaded (a word >= q_j is flagged, not fixed).  The words are fhe_keyswitch_apply's, bit for bit.
 * d_c is not sealed here: its consuming loads are inside the transform kernels of stage 0.
 * fhe_keyswitch_sealed_layout: out = {0, offset of the checked block = dnum 2 M, total, 1 if the plan takes the fused route}.
 * The fused kernel exists for dnum <= 12; above, stage 3 is the verifying sweep over the key's rows followed by the checked inner
 * product, writing the same flag words (a NULL d_seal_key is then not swept at all).
 * FHE_ERR_INVALID / FHE_ERR_UNSUPPORTED with nothing launched and the flag buffer untouched: outside fhe_keyswitch_apply_checked's
 * scope, a NULL argument, d_out0 == d_out1, a buffer that is not 16-byte aligned, a hook outside the call.  No repairing form:
 * repair needs the sweep.
 *
 * fhe_rotate_sealed_fused: fhe_rotate_sealed (same arguments, flag layout fhe_rotate_sealed_layout, same words) with the key's sweep
 * gone and stage 3 as above, which writes the key rows' flags where the sweep wrote them; the sweeps over c0 and c1 stay.
 * fhe_hmult_sealed_fused_key: fhe_hmult_sealed_fused (same arguments, flag layout fhe_hmult_sealed_layout, same words) with the key
 * fused as well: no input is swept at all.
 * Not covered on the consuming load: the plan's digits (ext) and the input limbs, which the inner product also loads; the prepared
 * keys of hoisted rotations and the giant keys of the BSGS product; sharded plans.
 * Test hook: fhe_ctx_inject_fault_keyswitch_sealed(key_row, coeff, bit), key_row = (d 2 + h) M + j, negative clears; taken, one
 * shot and whatever the outcome, by the next of the three calls above.  The bit of that key word is flipped in the register as
 * loaded, before window, digest and product read it; memory stays clean.  A key row or coeff outside the call that takes it, or a
 * plan above the fused cap (there is no fused load to hit), makes that call return FHE_ERR_INVALID with nothing launched.  The
 * sweep-based calls do not take the hook. */
int fhe_keyswitch_sealed_layout(const fhe_keyswitch *p, int out[4]);
int fhe_keyswitch_apply_sealed(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c, const uint64_t *d_evk,
                               const uint64_t *d_add0, const uint64_t *d_add1, const fhe_abft *a, const uint64_t *d_seal_key, uint32_t *d_flags,
                               void *stream);
int fhe_rotate_sealed_fused(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1,
                            uint32_t galois_elt, const uint64_t *d_galois_key, const fhe_abft *a, const uint64_t *const *d_seal_in,
                            const uint64_t *d_seal_key, uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream);
int fhe_hmult_sealed_fused_key(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_a0, const uint64_t *d_a1,
                               const uint64_t *d_b0, const uint64_t *d_b1, const uint64_t *d_relin_key, int rescale, const fhe_abft *a,
                               const uint64_t *const *d_seal_in, const uint64_t *d_seal_key, uint64_t *const *d_seal_out, uint32_t *d_flags,
                               void *stream);
int fhe_ctx_inject_fault_keyswitch_sealed(fhe_ctx *ctx, int key_row, long long coeff, int bit);

/* ---- sealed Galois permutation and sealed hoisted rotations: the source verified on the permutation's own gather -------------
 * fhe_automorphism_ntt_checked compares two residue sums modulo 2^32 - 1 (blind to +2^b - 2^(b+32) inside a word) from two reads of
 * the source, and says nothing about a word that was already wrong in memory.  A permutation gathers each source word exactly
 * once, so here the register that is stored is the register that is digested with the sums of fhe_seal (modulo 2^61 - 1): with its
 * SOURCE weight against the source's seal, with its DESTINATION weight for the destination's seal.  16 N bytes per row against the
 * 40 N of fhe_seal_verify + fhe_automorphism_ntt_checked + fhe_seal.
 *
 * fhe_automorphism_ntt_sealed: d_dst = sigma_k(d_src) over the rows [n_poly][limbs] of table limbs start_idx .. (fhe_seal's row
 * convention), out of place, both buffers 16-byte aligned, galois_elt odd.  d_seal_src ([rows][2], required: without it nothing
 * would check the permutation) is held word for word against the digest of the words as gathered; d_flags [rows], cleared by the
 * call, with fhe_seal_verify's bits (1 the row as gathered is not the row that was sealed, 2 a word >= q_l).  d_seal_dst ([rows][2],
 * may be NULL, may be d_seal_src) receives {S0 as STORED in d_seal_src, the digested S1 of the destination}: S0 is carried, since a
 * permutation leaves it alone, so a row whose S0 moved on this call's load keeps failing every later verification of d_dst.  The
 * hole that is left: a source change that keeps S0 and moves S1 alone raises the source's flag here but does not poison
 * d_seal_dst.  On clean data the words are fhe_automorphism_ntt's, bit for bit; a raised flag does not stop the stores.
 *
 * fhe_rotate_hoisted_sealed: fhe_rotate_hoisted_checked (its arguments first, CKKS form only) with the operands protected at rest.
 * d_seal_in = HOST [2] the seals of c0, c1 ([L][2] each; the array or an entry may be NULL); d_seal_keys = HOST [n_rot] the seals of
 * the PREPARED keys ([dnum 2 M][2], fhe_seal over the key as [dnum 2][M] rows; the array or an entry may be NULL); d_seal_out0 /
 * d_seal_out1 = HOST [n_rot] each, where the outputs' seals go ([L][2]; NULL: not sealed).  Flags, cleared by the call:
 *     [c1 rows L][per rotation r: [c0 rows L][key rows dnum 2 M]][fhe_rotate_hoisted_checked's block, exactly its layout]
 * c1 is verified once by a sweep (its consuming load is inside the transform kernels of stage 0).  Per rotation the inner product
 * verifies the prepared key on the load that multiplies it (as fhe_keyswitch_apply_sealed; above 12 digits a sweep followed by the
 * checked inner product), and with c0's seal the L rows of c0 go through the sealed permutation: EVERY rotation verifies c0 on its
 * own gather, no sweep over c0 exists, the verdict lands in that rotation's [c0 rows] and the c0 words of the checked block's
 * permutation stage stay zero.  With a NULL c0 seal c0 goes through the checked permutation exactly as in the checked call and the
 * [c0 rows] stay zero.  A raised input flag does not stop the call.  Words are fhe_rotate_hoisted's, bit for bit.
 * fhe_rotate_hoisted_sealed_layout: out = {offset of the c1 rows = 0, offset of rotation 0's input block = L, words per rotation
 * input block = L + dnum 2 M, offset of the checked block, total, 1 if the keys take the fused route}.
 * Not covered on the consuming load: c1; sigma(c0), which sits in the plan and is re-read by the tail; the sums; BGV and sharded
 * plans; no repairing form.
 *
 * Test hook: fhe_ctx_inject_fault_galois_sealed(rot, point, row, coeff, bit), a negative point clears; taken, one shot and whatever
 * the outcome, by the next of the two calls above.  Point 0 flips the bit of the word gathered for destination word coeff of `row`
 * in the register, before both digests and the store; point 1 flips a bit (< log N) of its source index, before the load and before
 * the source weight is formed.  rot names the rotation of the hoisted call, row a row of c0; the standalone call takes rot = 0 only.
 * A rotation, row or word outside the call, point 1 with bit >= log N, or a NULL c0 seal in the hoisted call make that call return
 * FHE_ERR_INVALID with nothing launched.  fhe_rotate_hoisted_sealed also takes fhe_ctx_inject_fault_rotate_hoisted's hook; a
 * permutation-stage fault on a c0 row is refused when c0's seal is given.  The checked calls do not take this hook. */
int fhe_automorphism_ntt_sealed(fhe_ctx *ctx, uint64_t *d_dst, const uint64_t *d_src, uint64_t *d_seal_dst, const uint64_t *d_seal_src,
                                const fhe_ntt_tables *t, size_t n_poly, size_t limbs, size_t start_idx, uint32_t galois_elt, uint32_t *d_flags,
                                void *stream);
int fhe_rotate_hoisted_sealed_layout(const fhe_keyswitch *p, size_t n_rot, int out[6]);
int fhe_rotate_hoisted_sealed(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *const *d_out0, uint64_t *const *d_out1, const uint64_t *d_c0,
                              const uint64_t *d_c1, const uint32_t *galois_elts, const uint64_t *const *d_prepared_keys, size_t n_rot,
                              const fhe_abft *a, const uint64_t *const *d_seal_in, const uint64_t *const *d_seal_keys,
                              uint64_t *const *d_seal_out0, uint64_t *const *d_seal_out1, uint32_t *d_flags, void *stream);
int fhe_ctx_inject_fault_galois_sealed(fhe_ctx *ctx, int rot, int point, int row, long long coeff, int bit);

/* ---- sealed inverse NTT: the input limbs of a key switch verified on the transform's own load --------------------------------
 * fhe_keyswitch_apply_sealed does not seal d_c, and the sealed rotations sweep c0 and c1 and then move them through the unchecked
 * permutation: the verifying sweep, the copy into the plan's coefficient buffer and the opening inverse transform's load are
 * separate loads.  A word that is wrong on the copy's load or on the transform's own load passes the seal and is a consistent input
 * of the ABFT identity (the input-side sum is formed from the word as loaded): a wrong result and no flag.  Here the first launch of
 * the checked inverse transform digests every raw 64-bit word its first register step takes -- the sums of fhe_seal, modulo
 * 2^61 - 1, weight = index in the row plus one, and the window word < q_l -- before the word is converted and enters the
 * butterflies, and a finish launch holds each row's two sums word for word against the stored seal.
 *
 * fhe_ntt_inverse_sealed: d_dst = the words of fhe_ntt_inverse_batch over d_src's rows [n_poly][limbs] of table limbs start_idx ..,
 * bit for bit; d_dst == d_src is allowed (in place), otherwise the transform is out of place with no copy and d_src is only read.
 * d_seal_src ([rows][2], fhe_seal's; NULL: not compared, the window still is).  d_flags [2][rows], cleared by the call: block 0 the
 * seal verdict per row with fhe_seal_verify's bits (1 the row as the transform loaded it is not the row that was sealed, or a
 * stored sum is not canonical; 2 a word >= q_l), block 1 fhe_ntt_inverse_checked's flag.  A raised seal flag does not stop the
 * call: the words are then the transform of the row as loaded.  Scope: fhe_ntt_inverse_checked's fused scope (N >= 2^5, not with
 * ntt_mode=1, ntt_resident, ntt_packed or a single-pass hook), FHE_ERR_UNSUPPORTED with nothing launched outside it.  The call
 * always runs whole-batch launches: a batch that fhe_ntt_inverse_checked would cut into sub-batches is NOT cut here.  It takes
 * fhe_ctx_inject_fault's flip between the two launches as fhe_ntt_inverse_checked does (N >= 2^13; the index counts from d_dst).
 *
 * fhe_keyswitch_apply_sealed_in: fhe_keyswitch_apply_sealed with d_c sealed as well.  d_seal_c ([L][2], required: a NULL is refused,
 * since nothing would verify the input -- the refused call still takes an armed hook) comes before d_seal_key.  Stage 0 is: no
 * copy, the sealed inverse out of place from d_c into the plan's coefficient buffer; its ABFT verdict goes where stage 0's goes,
 * its seal verdict to the c rows.  Flags, cleared by the call:
 *     [c rows L][key rows dnum 2 M][the checked key switch's own block, exactly its layout]
 * fhe_keyswitch_sealed_in_layout: out = {0, offset of the key rows = L, offset of the checked block, total, 1 if the key takes the
 * fused route}.  CKKS or BGV form by the plan's plain modulus; the words are fhe_keyswitch_apply's.  Refusals as
 * fhe_keyswitch_apply_sealed's, with nothing launched and the flag buffer untouched.
 *
 * fhe_rotate_sealed_in: fhe_rotate_sealed_fused's arguments (d_seal_in = HOST [2] the seals of c0, c1, both required) with no sweep
 * over c0 or c1 and no unchecked permutation: both go through the sealed Galois permutation (fhe_automorphism_ntt_sealed's
 * kernel), c0 verified on the gather, c1 verified on the gather while sigma(c1)'s seal {carried S0, digested S1} is written into
 * call scratch from the registers that are stored; stage 0 then verifies sigma(c1) against that seal on the transform's load.  The
 * key is verified on the fused inner product, the outputs are sealed as in fhe_rotate_sealed.  Flags, cleared by the call:
 *     [c0 rows L][c1 rows L][sigma(c1) rows L][key rows dnum 2 M][the checked key switch's own block]
 * fhe_rotate_sealed_in_layout: out = {offsets of the c0 rows, c1 rows, sigma(c1) rows, key rows, checked block, total, 1 if the key
 * takes the fused route}.  A c1 word corrupted at rest raises c1's row and, through the carried S0, sigma(c1)'s row.  The words are
 * fhe_rotate's.
 *
 * Not covered: the inner product's own load of the input limbs d_c and of the digits (ext); sigma(c0), which the tail re-reads
 * from the plan; hoisted rotations and the BSGS product (their front half can take the same step later); sharded plans; repair;
 * sub-batched streaming batches.
 *
 * Test hook: fhe_ctx_inject_fault_ntt_sealed(row, coeff, bit), a negative row clears; taken, one shot and whatever the outcome, by
 * the next of the three calls above (row = a row of the transform: of d_src, of d_c, of sigma(c1)).  The bit of that word is flipped
 * in the register as loaded, before window, digest and conversion; memory stays clean.  A row or coeff outside the call that takes
 * it makes that call return FHE_ERR_INVALID with nothing launched.  Calls that do not run the sealed transform do not take it. */
int fhe_ntt_inverse_sealed(fhe_ctx *ctx, uint64_t *d_dst, const uint64_t *d_src, const fhe_ntt_tables *t, const fhe_abft *a, size_t n_poly,
                           size_t limbs, size_t start_idx, const uint64_t *d_seal_src, uint32_t *d_flags, void *stream);
int fhe_ctx_inject_fault_ntt_sealed(fhe_ctx *ctx, int row, long long coeff, int bit);
int fhe_keyswitch_sealed_in_layout(const fhe_keyswitch *p, int out[5]);
int fhe_keyswitch_apply_sealed_in(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c, const uint64_t *d_evk,
                                  const uint64_t *d_add0, const uint64_t *d_add1, const fhe_abft *a, const uint64_t *d_seal_c,
                                  const uint64_t *d_seal_key, uint32_t *d_flags, void *stream);
int fhe_rotate_sealed_in_layout(const fhe_keyswitch *p, int out[7]);
int fhe_rotate_sealed_in(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1,
                         uint32_t galois_elt, const uint64_t *d_galois_key, const fhe_abft *a, const uint64_t *const *d_seal_in,
                         const uint64_t *d_seal_key, uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream);

/* ---- sealed forward NTT: input verified on load, output sealed on store; the sealed inverse with an output seal --------------
 * fhe_ntt_forward_checked forms its input-side ABFT sum from the word as loaded, so a word corrupted at rest -- the experiment of
 * reliability_test/ntt_test.cu:104-144 -- is a consistent input: no flag, every output word wrong.  The composition fhe_seal_verify
 * + fhe_ntt_forward_checked + fhe_seal verifies on one load, transforms from another and seals the output by re-reading it after
 * the store.  Here the launch that loads the transform's input (the forward column pass; below 2^13 the single pass) digests every
 * raw 64-bit word its first register step takes, as fhe_ntt_inverse_sealed does, and the launch that stores the result digests
 * every final word on its way to memory with weight = its index in the stored row plus one: the seal of fhe_seal over the output
 * row, word for word.  A change of domain keeps its chain of custody.
 *
 * fhe_ntt_forward_sealed: d_dst = the words of fhe_ntt_forward_batch over d_src's rows [n_poly][limbs] of table limbs start_idx ..,
 * bit for bit -- also for a source word >= q_l, which is digested as it is, raises bit 2 and is reduced as the unchecked transform
 * reduces it.  d_dst == d_src runs in place, otherwise out of place with no copy and d_src is only read.  d_seal_src ([rows][2],
 * fhe_seal's; NULL: not compared, the window still is).  d_seal_dst ([rows][2]; NULL: nothing is written and no output digest is
 * launched).  d_flags [2][rows], cleared by the call: block 0 the input seal verdict per row with fhe_seal_verify's bits, block 1
 * fhe_ntt_forward_checked's flag.  A raised flag does not stop the call.
 * fhe_ntt_inverse_sealed_out: the same arguments and rules over fhe_ntt_inverse_batch's words and fhe_ntt_inverse_checked's flag;
 * with d_seal_dst == NULL it is fhe_ntt_inverse_sealed.
 *
 * The poison rule: d_seal_dst[row] is the canonical digest of the stored row where the row's word in block 0 and its word in block
 * 1 are both zero, and {~0, ~0} otherwise.  A stored sum that is not canonical differs from every digest in every verifier, so a
 * row with any raised flag leaves the call with a seal that can never verify: it stays raised in every later verification and
 * fhe_seal_repair reports it FHE_SEAL_UNCORRECTABLE.
 *
 * Scope and refusals are fhe_ntt_inverse_sealed's: N >= 2^5, not with ntt_mode=1, ntt_resident, ntt_packed or a single-pass hook
 * (FHE_ERR_UNSUPPORTED with nothing launched and the flag buffer untouched); whole-batch launches only.  Both calls take
 * fhe_ctx_inject_fault's flip between the two launches at N >= 2^13, as the checked transforms do, and
 * fhe_ctx_inject_fault_ntt_sealed, one shot and whatever the outcome: the bit of that input word is flipped in the register as
 * loaded, memory stays clean; a row or word outside the call gives FHE_ERR_INVALID with nothing launched.
 *
 * Not covered: a fault between the tap's read of a register and the conversion that consumes it; the hand-off between the two
 * launches beyond what the whole-transform ABFT sum sees; sub-batched streaming batches; the forward transforms inside the key
 * switch (stages 2 and 6), which stay the checked ones; repair; sharded plans.  (The negacyclic product has a sealed call of its
 * own, fhe_polymul_sealed below.) */
int fhe_ntt_forward_sealed(fhe_ctx *ctx, uint64_t *d_dst, const uint64_t *d_src, const fhe_ntt_tables *t, const fhe_abft *a, size_t n_poly,
                           size_t limbs, size_t start_idx, const uint64_t *d_seal_src, uint64_t *d_seal_dst, uint32_t *d_flags, void *stream);
int fhe_ntt_inverse_sealed_out(fhe_ctx *ctx, uint64_t *d_dst, const uint64_t *d_src, const fhe_ntt_tables *t, const fhe_abft *a, size_t n_poly,
                               size_t limbs, size_t start_idx, const uint64_t *d_seal_src, uint64_t *d_seal_dst, uint32_t *d_flags, void *stream);

/* ---- sealed rescale and sealed tail: inputs verified on load, outputs sealed on store ------------------------------------------
 * fhe_rescale_checked and fhe_bgv_mod_switch_checked do not cover faults already in their input, and every sealed composite seals
 * its outputs with a sweep after its last launch: a word corrupted between the final store and that sweep's load is sealed as it
 * is.  The last launch of a key switch (stage 7) and of a rescale (stage 3) is the same kernel, which loads each word of its first
 * operand once and stores each result word once.  Its sealed form digests the operand from the register it subtracts from (IN) and
 * the result from the register it stores (OUT) -- the sums of fhe_seal, modulo 2^61 - 1, weight = index in the row plus one, and
 * the window word < q_l -- and a finish launch holds the input rows' sums word for word against their stored seals and writes the
 * output rows' seals.  The arithmetic, the words, the residue flags and their place are the checked tail's.
 *
 * fhe_rescale_sealed: fhe_rescale_checked's arguments (the CKKS or the BGV form by the plan's plain modulus) with d_seal_in
 * ([n_parts][L][2], fhe_seal's, required) and d_seal_out ([n_parts][L - 1][2], required, written).  Stage 0 makes no copy: each
 * part's last limb goes through the sealed inverse transform (fhe_ntt_inverse_sealed's kernel) out of place from d_in into the
 * plan; stages 1, 2, 4, 5 are the checked rescale's; stage 3 is the sealed tail, IN and OUT.  Flags, cleared by the call:
 *     [input rows n_parts L][the checked rescale's own block, exactly its layout]
 * input words with fhe_seal_verify's bits: rows 0 .. L - 2 of a part from stage 3's load, row L - 1 from stage 0's.  A raised
 * input flag does not stop the call.  fhe_rescale_sealed_layout: out = {0, offset of the checked block = n_parts L, total, 0}.
 * Out of place only, 16-byte aligned buffers, N >= 2; a NULL seal argument, an overlap or a sharded plan is refused with nothing
 * launched and the flag buffer untouched.  The words are fhe_rescale's, bit for bit -- also for an input word >= q_l: it is
 * flagged (bit 2 on its row, bit 4 in the stage-3 word), not fixed.
 *
 * fhe_hmult_sealed_out: fhe_hmult_sealed_fused_key's arguments, flag layout and words, without the two output sweeps: the last
 * launch -- the key switch's stage 7, or with rescale the rescale's stage 3 -- is the sealed tail in its OUT form and writes
 * d_seal_out[0], d_seal_out[1] (an entry that is NULL is not written).  fhe_rotate_sealed_out: the same for fhe_rotate_sealed_in.
 *
 * Not covered: the tail's second operand (the plan's own residues) and its addends (plan-internal in these calls, the caller's
 * own in fhe_keyswitch_apply_*) are not digested; a fault after the output's digest (the store, memory) is caught by whoever
 * verifies the seal next; repair and locators; sharded plans; the hoisted rotations' and the BSGS product's tails.
 *
 * Test hook: fhe_ctx_inject_fault_subscale_sealed(point, row, coeff, bit), a negative point clears; taken, one shot and whatever
 * the outcome, by the next of the three calls above.  Point 0 flips the bit of an input word in the register as loaded, before
 * window, digest and arithmetic (row = part * L + l, l < L - 1; fhe_rescale_sealed only); point 1 flips the bit of an output word
 * in the register after its digest and before its store (row = part * limbs + l of the outputs).  A row or word outside the call,
 * point 0 in a call without the input step, a last-limb row, or point 1 without output seals makes that call return
 * FHE_ERR_INVALID with nothing launched.  Calls that do not run the sealed tail do not take it.  fhe_rescale_sealed also takes
 * fhe_ctx_inject_fault_ntt_sealed (row = a last-limb row part * L + L - 1) and the checked rescale's own hook of its form. */
int fhe_ctx_inject_fault_subscale_sealed(fhe_ctx *ctx, int point, int row, long long coeff, int bit);
int fhe_rescale_sealed_layout(const fhe_keyswitch *p, size_t n_parts, int out[4]);
int fhe_rescale_sealed(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out, const uint64_t *d_in, size_t n_parts, const fhe_abft *a,
                       const uint64_t *d_seal_in, uint64_t *d_seal_out, uint32_t *d_flags, void *stream);
int fhe_hmult_sealed_out(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_a0, const uint64_t *d_a1,
                         const uint64_t *d_b0, const uint64_t *d_b1, const uint64_t *d_relin_key, int rescale, const fhe_abft *a,
                         const uint64_t *const *d_seal_in, const uint64_t *d_seal_key, uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream);
int fhe_rotate_sealed_out(fhe_ctx *ctx, fhe_keyswitch *p, uint64_t *d_out0, uint64_t *d_out1, const uint64_t *d_c0, const uint64_t *d_c1,
                          uint32_t galois_elt, const uint64_t *d_galois_key, const fhe_abft *a, const uint64_t *const *d_seal_in,
                          const uint64_t *d_seal_key, uint64_t *const *d_seal_out, uint32_t *d_flags, void *stream);

/* ---- sealed negacyclic product: factors verified on load, product sealed on store ----------------------------------------------
 * fhe_polymul_checked forms its input-side sums from the words as loaded: a bit that rots in a factor at rest -- the fault model of
 * reliability_test/ntt_test.cu:104-144 and dotprod_test.cu:31-61 -- is a consistent input to all three identities: no flag, every
 * word of c wrong.  The composition fhe_seal_verify(a) + fhe_seal_verify(b) + fhe_polymul_checked + fhe_seal(c) verifies each factor
 * on one load and consumes it on another, leaves c unsealed between its final store and the sweep's load, and reads a and b twice
 * and c once more than needed.  Here the launch that loads a factor (its forward column pass; below 2^13 the single launch that is
 * the whole product) digests every raw 64-bit word its first register step takes and holds it against the window, and the launch
 * that stores c (the inverse column pass; below 2^13 the same single launch) digests every final word on its way to memory.
 *
 * fhe_polymul_sealed: the data contract of fhe_polymul and fhe_polymul_checked -- rows [n_poly][limbs] of table limbs start_idx ..,
 * c may alias either factor, a and b are SCRATCH: AFTER THE CALL d_seal_a AND d_seal_b NO LONGER DESCRIBE d_a AND d_b.  The words of
 * c are fhe_polymul's, bit for bit -- also for a factor word >= q_l, which is flagged, not fixed.  rows = n_poly limbs, row (poly, l)
 * = poly limbs + l.  d_flags, uint32 [rows a][rows b][rows][3] = 5 rows words, cleared by the call: block 0 a's seal verdict per row
 * and block 1 b's, with fhe_seal_verify's bits (a NULL seal is not compared, the window always is); block 2 fhe_polymul_checked's
 * own block, exactly its layout and meaning.  A raised input flag does not stop the call.  d_a == d_b is squaring: one forward
 * transform, d_seal_b must be NULL or d_seal_a (anything else: FHE_ERR_INVALID), block 1 repeats block 0.  d_seal_c ([rows][2]; NULL:
 * no output digest) equals fhe_seal(c) word for word on a row with no raised flag; the poison rule applies otherwise: a row with its
 * a-verdict, its b-verdict or any of its three ABFT words raised leaves with {~0, ~0}, a seal that can never verify.
 *
 * Refused with nothing launched and the flag buffer untouched: FHE_ERR_UNSUPPORTED for ntt_mode=1, ntt_resident, ntt_packed, a
 * single-pass hook, N < 2^5, a table set without an inverse; FHE_ERR_INVALID for a detector made for another table set, a NULL
 * d_a / d_b / d_c / d_flags, buffers that are not 16-byte aligned.  Whole-batch launches only: no sub-batch cut, no side streams.
 *
 * Test hooks, both taken one shot and whatever the call's outcome (a refused call takes them with it): fhe_ctx_inject_fault_polymul's
 * points 0-3 as in the checked call (2 at every size, 0 / 1 / 3 from 2^13 on) -- they poison the row's output seal through block 2 --
 * and fhe_ctx_inject_fault_polymul_sealed(operand, row, coeff, bit), operand 0 = a, 1 = b, negative clears: the bit of word coeff of
 * that factor's row is flipped in the register as the loading launch takes it, before window, digest and conversion; memory stays
 * clean.  A row or word outside the call, or operand 1 when squaring: FHE_ERR_INVALID with nothing launched.  fhe_polymul_checked
 * does not run the step: it leaves the hook armed and sees nothing.
 *
 * Not covered: a fault between the tap's read of a register and the conversion that consumes it; the hand-offs between the launches
 * beyond what the ABFT sums see; sub-batched streaming batches; repair (it needs the sweep); sharded plans; ntt_mode=1; N < 2^5. */
int fhe_ctx_inject_fault_polymul_sealed(fhe_ctx *ctx, int operand /* 0 = a, 1 = b, < 0 disarms */, int row, long long coeff, int bit);
int fhe_polymul_sealed(fhe_ctx *ctx, uint64_t *d_c, uint64_t *d_a, uint64_t *d_b, const fhe_ntt_tables *t, const fhe_abft *a,
                       size_t n_poly, size_t limbs, size_t start_idx,
                       const uint64_t *d_seal_a, const uint64_t *d_seal_b, uint64_t *d_seal_c, uint32_t *d_flags, void *stream);

/* ---- fault injection ---------------------------------------------------------------- */
/* _flip_bit_kernel<<<1,1>>> (reliability_test/dotprod_test.cu:31-33,55): data[idx] ^= 1 << bit */
int fhe_flip_bit(fhe_ctx *ctx, uint64_t *d_data, uint64_t idx, int bit, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FHE_MI355X_H */
