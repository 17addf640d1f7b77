"""Inputs of the streaming-kernel tests (tests/test_stream_cases.py, tests/test_gpu_stream_products.py, tests/test_gpu_long_grids.py):
products that need the conditional subtraction behind the 128-bit Barrett step, and the shapes at which every capped grid takes a
second trip through its grid-stride loop.  Pure Python: importable without a GPU.

The Barrett step.  barrett128() (csrc/modarith.hpp) estimates the quotient of x = hi 2^64 + lo by q as
qhat = floor(x floor(2^128 / q) / 2^128) (the low word of lo * r0 that it drops cannot carry into the floor).  The estimate is
floor(x / q) or one short -- never two: tests/test_stream_cases.py derives it -- and it is one short exactly when x mod q is small
against x (2^128 mod q) / 2^128: only then does `r = r >= q ? r - q : r` change the word.  barrett128() carries that line twice,
"for robustness"; since the estimate is never two short, either one alone does the work and only the removal of both is visible.
Random canonical operands never get there (for a 50-bit prime the residue would have to fall below about 2^-28 q); the pairs built
here do, by construction: b = s a^-1 mod q has a b mod q = s for s = 1, 2, 3.  barrett_shortfall() restates the estimate, so that
tests/test_stream_cases.py can say for every modulus whether the family reaches the subtraction (it cannot for 30-bit primes and
canonical words: x < 2^60 makes the correction term smaller than 1 / q).

The grids.  GRID_CAPS lists every streaming launcher's cap as it stands in the sources today, the elements one lane takes per trip
and so the stride of the loop, and LONG_CASES the shape of tests/test_gpu_long_grids.py that passes it -- with the trips that shape
takes.  Nothing asserts the launcher's rule: a launcher may change its cap, the table then names the case to look at again.

  launcher (source)                                            cap            per lane   stride of one trip
  k_modmul, plain / acc / non-temporal (aux_kernels)            8192 x 256     2 words    4 194 304 words
  k_modmul_checked (pointwise_checked)                          8192 x 256     2 words    4 194 304 words (= 16384 x 256)
  k_modadd, k_modsub, k_scalar_affine (aux_kernels)             8192 x 256     1 word     2 097 152 words
  k_automorphism, k_automorphism_ntt (aux_kernels)              8192 x 256     1 word     2 097 152 words
  k_modadd_checked (bsgs_checked)                               8192 x 256     1 word     2 097 152 words
  k_scalar_affine_checked (scalar_checked)                      8192 x 256     1 word     2 097 152 words
  k_automorphism_ntt_checked (galois_checked)                   none: one workgroup per chunk of the batch, no stride loop
  k_tensor, k_tensor_checked (aux_kernels, pointwise_checked)   16384 x 256    1 word     4 194 304 words
  k_bconv_fast (+ checked), k_crt_garner, k_bsgs_hadamard       4096 x 256     1 column   1 048 576 columns
  k_row_digest (seal, verify), k_row_locator                    8192 jobs      1 (row, chunk) job per workgroup
  k_modadd_carry, k_automorphism_ntt_sealed, k_tensor_sealed    8192 jobs      1 (row, chunk) job per workgroup; their long cases are
                                                                               test_the_job_loop_takes_a_second / a_fourth_trip of their own files
  k_mac_sealed (both families)                                  8192 jobs      not listed: their rows are limbs, a few dozen at most, times
                                                                               at most 16 chunks -- no plan reaches the cap
  k_row_repair                                                  2048 rows      1 row per workgroup
"""
import numpy as np

M64 = (1 << 64) - 1


def barrett_qhat(x, q):
    """barrett128()'s quotient estimate for the 128-bit x, word for word: the same 64-bit products, the dropped low word of lo * r0,
    the two carries, the wrap of the sum to 64 bits"""
    ratio = (1 << 128) // q
    r0, r1 = ratio & M64, ratio >> 64
    assert r1 <= M64
    lo, hi = x & M64, x >> 64
    c = (lo * r0) >> 64                              # mulhi64(lo, r0): the low word of this product is dropped
    t1l, t1h = (lo * r1) & M64, (lo * r1) >> 64
    t2l, t2h = (hi * r0) & M64, (hi * r0) >> 64
    s = (t1l + t2l) & M64
    carry = int(s < t1l)
    s2 = (s + c) & M64
    carry += int(s2 < s)
    return (hi * r1 + t1h + t2h + carry) & M64


def barrett_shortfall(x, q):
    """x // q - qhat (as 64-bit words: the kernel forms lo - qhat q modulo 2^64): how many times q still has to be subtracted"""
    d = (x // q - barrett_qhat(x, q)) & M64
    return d - (1 << 64) if d >> 63 else d


def barrett128(x, q):
    """the word barrett128() returns for x: the estimate's remainder with the two conditional subtractions"""
    r = ((x & M64) - barrett_qhat(x, q) * q) & M64
    for _ in range(2):
        r = r - q if r >= q else r
    return r


def lift(v, q):
    """the largest 64-bit word congruent to v modulo q"""
    return v + (M64 - v) // q * q


def residue_pairs(q, n, rng, residues, lifted=False):
    """n pairs (a, b) with a drawn from [q/2, q) and b = s a^-1 mod q, s running through `residues`: a b mod q = s.  lifted: both
    replaced by the largest 64-bit words of their residue classes"""
    out = []
    for i in range(n):
        a = int(rng.integers(q // 2, q))
        b = residues[i % len(residues)] % q * pow(a, -1, q) % q
        out.append((lift(a, q), lift(b, q)) if lifted else (a, b))
    return out


def special_pairs(q, lifted=False):
    """the fixed pairs mixed into the family: (q - 1, q - 1) and (1, 1), whose products are 1 modulo q, and -- among the lifted pairs
    only, a lone q is not canonical -- the products that are exactly q, 2q and q (q - 1)"""
    if not lifted:
        return [(q - 1, q - 1), (1, 1)]
    return [(lift(q - 1, q), lift(q - 1, q)), (lift(1, q), lift(1, q)), (q, 1), (2, q), (q, q - 1)]


def small_residue_pairs(q, n, rng, lift=False):
    """n pairs (a, b) whose product is 1, 2 or 3 modulo q (0 for the exact multiples among the lifted specials): the specials first,
    then the family b = s a^-1.  Canonical words unless `lift`; zero factors and a lone q paired with an arbitrary word are
    test_gpu_pointwise_plain.py's _edge_pairs"""
    sp = special_pairs(q, lift)[:n]
    return sp + residue_pairs(q, n - len(sp), rng, (1, 2, 3), lift)


def fp64_edge_pairs(q, n, rng):
    """canonical pairs for the FP64 limbs of the tensor product: a b mod q next to 0 from above (1, 2, 3) and from below (q - 1, q - 2),
    the two ends at which ArithF64::canonical()'s sign fix decides the word"""
    return residue_pairs(q, n, rng, (1, q - 1, 2, q - 2, 3))


def garner_python(res, mods):
    """k_crt_garner's recurrence in Python integers (prefix products and every product wrapped to 128 bits, the first digit taken
    as it is)"""
    M128 = (1 << 128) - 1
    pref = [1]
    for p in mods[:-1]:
        pref.append(pref[-1] * p & M128)
    lo, hi = [], []
    for col in np.asarray(res).T.tolist():
        c = [col[0]]
        for j in range(1, len(mods)):
            p = mods[j]
            t = col[j] % p
            for kk in range(j):
                t = (t - (c[kk] * pref[kk] & M128) % p) % p
            c.append(t * pow(pref[j] % p, -1, p) % p)
        x = sum(ck * pk for ck, pk in zip(c, pref)) & M128
        lo.append(x & M64)
        hi.append(x >> 64)
    return np.array(lo, dtype=np.uint64), np.array(hi, dtype=np.uint64)


# ---- the grids ------------------------------------------------------------------------------------------------------------------
# name -> (workgroups at the cap, elements per workgroup and trip, what an element is)
GRID_CAPS = {
    "modmul": (8192, 512, "word"),
    "modmul_checked": (8192, 512, "word"),
    "modadd": (8192, 256, "word"),
    "modsub": (8192, 256, "word"),
    "scalar_affine": (8192, 256, "word"),
    "modadd_checked": (8192, 256, "word"),
    "scalar_affine_checked": (8192, 256, "word"),
    "automorphism": (8192, 256, "word"),
    "automorphism_ntt": (8192, 256, "word"),
    "automorphism_ntt_checked": (None, None, "word"),          # no cap and no stride loop
    "tensor": (16384, 256, "word"),
    "tensor_checked": (16384, 256, "word"),
    "bconv_fast": (4096, 256, "column"),
    "bconv_fast_checked": (4096, 256, "column"),
    "crt_garner": (4096, 256, "column"),
    "bsgs_hadamard": (4096, 256, "column"),
    "seal": (8192, 1, "job"),
    "seal_verify": (8192, 1, "job"),
    "seal_locator": (8192, 1, "job"),
    "modadd_sealed": (8192, 1, "job"),
    "automorphism_ntt_sealed": (8192, 1, "job"),
    "tensor_product_sealed": (8192, 1, "job"),
    "seal_repair": (2048, 1, "row"),
}


def stride(name):
    cap, per, _ = GRID_CAPS[name]
    return None if cap is None else cap * per


def trips(name, elements):
    """trips the busiest workgroup takes through its loop at the table's cap, and whether the last trip is partial"""
    s = stride(name)
    if s is None:
        return 1, False
    return -(-elements // s), elements % s != 0


POINTWISE_LOGN = 12
COLUMNS = 1572867                 # 1.5 trips of 4096 x 256 columns, odd
HADAMARD_K, HADAMARD_BS = 3, 524289
# name of the case in tests/test_gpu_long_grids.py -> (launchers it runs, elements of each launch)
LONG_CASES = {
    "pointwise 3 x 256": (("modadd", "modsub", "scalar_affine", "modadd_checked", "scalar_affine_checked", "automorphism", "automorphism_ntt",
                           "automorphism_ntt_checked"), 3 * 256 << 12),                          # 3 145 728 words: 1.5 trips
    "modmul 3 x 512": (("modmul", "modmul_checked"), 3 * 512 << 12),                                # 6 291 456 words: 1.5 trips
    "modmul non-temporal 3 x 683": (("modmul",), 3 * 683 << 12),                                    # 8 392 704 words: 2 trips and 4096 words
    "tensor 97 limbs": (("tensor", "tensor_checked"), 97 << 16),                                    # 6 356 992 words: 1.52 trips
    "columns": (("bconv_fast", "bconv_fast_checked", "crt_garner"), COLUMNS),                       # 1.5 trips
    "hadamard": (("bsgs_hadamard",), HADAMARD_K * HADAMARD_BS),                                     # 1 572 867 outputs: 1.5 trips
    "seal 12285 rows": (("seal", "seal_verify", "seal_locator"), 7 * 1755),                         # 12 285 jobs: 1.5 trips
    "seal two chunks": (("seal", "seal_verify", "seal_locator"), 7 * 2),                            # 14 jobs: one trip, two chunks per row
    "repair 3073 rows": (("seal_repair",), 3073),                                                   # 1.5 trips
}


def sample_columns(n_row, row_offset, stride_words, rng, count=64):
    """`count` columns of a row of n_row words that begins at word `row_offset` of its batch: random ones, the row's first and last
    word, and the first and last word of every trip (multiples of the stride, and the words before them) that falls into the row"""
    cols = {0, n_row - 1}
    first = -(-row_offset // stride_words) * stride_words
    for b in range(first, row_offset + n_row + 1, stride_words):
        for g in (b - 1, b):
            if row_offset <= g < row_offset + n_row:
                cols.add(g - row_offset)
    while len(cols) < min(count, n_row):
        for c in rng.integers(0, n_row, count).tolist():
            if len(cols) < count:
                cols.add(c)
    return np.array(sorted(cols), dtype=np.int64)
