"""CPU emulation of the sealed inner sum of the BSGS product (tests/emu/emu_bsgs_seal.cpp compiles bsgs_seal.hpp, the per-pair step
and the per-row decision the kernels of bsgs_sealed.hip call, and runs one limb row's job loop): the per-baby-step digests equal
Python-integer sums of the diagonal rows whatever the chunking, the words equal the checked inner sum's (the emulation of
bsgs_check.hpp) and Python integers, and a row that is not the row that was sealed is flagged -- without a GPU.

Every expected value is a Python integer computed here.  No trial is filtered out."""
import ctypes as C

import numpy as np
import pytest

from helpers.emu_build import build_emu
from oracle import cport as O

p64 = C.POINTER(C.c_uint64)
p32 = C.POINTER(C.c_uint32)
P = (1 << 61) - 1
SUM, RANGE = 1, 2
OPERAND = 4
# (n, log_chunk): a row shorter than a workgroup; 2^13 as one chunk and cut smaller
CUTS = [(1 << 5, 5), (1 << 13, 13), (1 << 13, 10), (1 << 13, 6)]
# NB = 4 with one term, the edge of NB = 4, the first n1 of NB = 8, the edge of NB = 16 (two folds of the running sums)
N1S = [1, 4, 5, 16]
# (path, bits): the U64 form serves every limb, the FP64-term form only limbs below 2^50
PATHS = [("u64", 30), ("u64", 61), ("f64", 50)]
PRIMES = {(bits, n): O.gen_primes(n, bits, 1)[0] for bits in (30, 50, 61) for n in (1 << 5, 1 << 13)}
HEADERS = ("modarith.hpp", "residue_check.hpp", "baseconv_check.hpp", "keyswitch_check.hpp", "bsgs_check.hpp", "seal_check.hpp", "bsgs_seal.hpp")


@pytest.fixture(scope="module")
def emu():
    L = build_emu("libemu_bsgs_seal.so", ["emu_bsgs_seal.cpp"], HEADERS)
    L.emu_diag_mac_sealed.restype = C.c_int
    L.emu_diag_mac_sealed.argtypes = [p64, p64, p64, C.c_int, C.c_uint32, C.c_uint64, C.c_int, C.c_int, p64, C.c_int, C.c_uint32, C.c_int, p64, p64, p32, p64,
                                      p32]
    return L


@pytest.fixture(scope="module")
def checked():
    """the emulation of bsgs_check.hpp: the checked inner sum, element by element"""
    L = build_emu("libemu_bsgs_check.so", ["emu_bsgs_check.cpp"], HEADERS[:5])
    L.emu_diag_mac_checked.restype = C.c_int
    L.emu_diag_mac_checked.argtypes = [p64, p64, p64, C.c_int, C.c_size_t, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, p64, p64, p32, p32]
    return L


def _u(x):
    return np.ascontiguousarray(x, dtype=np.uint64)


def _p(a):
    return a.ctypes.data_as(p64)


def _f(a):
    return a.ctypes.data_as(p32)


def sums(x):
    """[S0, S1] of a row, Python integers"""
    row = [int(v) for v in x]
    return [sum(row) % P, sum((j + 1) * v for j, v in enumerate(row)) % P]


def seals(d):
    return [sums(r) for r in d]


def sealed(emu, d, y0, y1, q, path, log_chunk, seal, hit=(0, 0, -1)):
    """(w0, w1, residue flags [2], digests [n1][2], seal flags [n1]) of one limb row"""
    d, y0, y1 = _u(d), _u(y0), _u(y1)
    n1, n = d.shape
    seal = _u(np.array(seal, dtype=object).astype(np.uint64).reshape(-1))
    w0, w1 = np.full(n, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64), np.full(n, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    fl, sf = np.full(2, 0xFFFF, dtype=np.uint32), np.full(n1, 0xFFFF, dtype=np.uint32)
    dg = np.full(2 * n1, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    assert emu.emu_diag_mac_sealed(_p(d), _p(y0), _p(y1), n1, n, q, 0 if path == "f64" else 1, log_chunk, _p(seal), *hit, _p(w0), _p(w1), _f(fl), _p(dg),
                                   _f(sf)) == 0
    return w0, w1, fl.tolist(), [[int(dg[2 * b]), int(dg[2 * b + 1])] for b in range(n1)], sf.tolist()


def inner_checked(checked, d, y0, y1, q, path):
    """words and flags of the checked inner sum (bsgs_check.hpp) on the same operands"""
    d, y0, y1 = _u(d), _u(y0), _u(y1)
    n = d.shape[1]
    w0, w1 = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    f0, f1 = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    assert checked.emu_diag_mac_checked(_p(d), _p(y0), _p(y1), d.shape[0], n, q, 0 if path == "f64" else 1, 0, -1, 0, _p(w0), _p(w1), _f(f0), _f(f1)) == 0
    return w0, w1, int(np.bitwise_or.reduce(f0)), int(np.bitwise_or.reduce(f1))


def dot(d, y, q):
    """sum_b d_b y_b mod q per word, Python integers"""
    return [sum(int(d[b][i]) * int(y[b][i]) for b in range(len(d))) % q for i in range(len(d[0]))]


def operands(rng, q, n1, n):
    mk = lambda: np.stack([rng.integers(0, q, n, dtype=np.uint64) for _ in range(n1)])
    return mk(), mk(), mk()


@pytest.mark.parametrize("n1", N1S)
@pytest.mark.parametrize("path,bits", PATHS)
def test_digests_equal_python_sums_and_words_equal_the_checked_inner_sum(emu, checked, path, bits, n1):
    for n in (1 << 5, 1 << 13):
        q = PRIMES[bits, n]
        d, y0, y1 = operands(np.random.default_rng(bits * 100 + n1 + n), q, n1, n)
        # the extremes of the window in every diagonal row, first and last word
        d[:, 0], d[:, -1] = 0, q - 1
        want = seals(d)
        want_w = dot(d, y0, q), dot(d, y1, q)
        c0, c1, cf0, cf1 = inner_checked(checked, d, y0, y1, q, path)
        assert (cf0, cf1) == (0, 0) and c0.tolist() == want_w[0] and c1.tolist() == want_w[1]
        for nn, log_chunk in CUTS:
            if nn != n:
                continue
            w0, w1, fl, dg, sf = sealed(emu, d, y0, y1, q, path, log_chunk, want)
            assert dg == want, (n, log_chunk)
            assert sf == [0] * n1 and fl == [0, 0], (n, log_chunk)
            assert w0.tolist() == want_w[0] and w1.tolist() == want_w[1], (n, log_chunk)
            assert (w0 == c0).all() and (w1 == c1).all()


@pytest.mark.parametrize("path,bits", PATHS)
def test_one_or_two_changed_words_of_a_row_are_flagged_with_certainty(emu, checked, path, bits):
    for (n, log_chunk), n1 in zip(CUTS, (4, 5, 16, 1)):
        q = PRIMES[bits, n]
        rng = np.random.default_rng(bits + n + log_chunk)
        d, y0, y1 = operands(rng, q, n1, n)
        d = np.minimum(np.maximum(d, np.uint64(16)), np.uint64(q - 17))      # every word stays in the window whichever way a small change goes
        seal = seals(d)
        # one word: a single bit, a multi-bit change the fold modulo 2^32 - 1 cannot see (bits below 30 and their images 32 up do
        # not both fit a 30-bit window: there it is a plain difference), the first and the last word of the row
        for b, j, delta in ((0, 0, 1), (n1 - 1, n - 1, -1), (n1 // 2, n // 2 + 1, 1 << 3), (0, 7, (1 << 35) - (1 << 3) if bits > 40 else 12345)):
            now = d.copy()
            v = int(d[b][j]) + delta
            if not 0 <= v < q:
                v = int(d[b][j]) - delta
            assert 0 <= v < q and v != int(d[b][j])
            now[b][j] = v
            w0, w1, fl, dg, sf = sealed(emu, now, y0, y1, q, path, log_chunk, seal)
            assert sf == [SUM if r == b else 0 for r in range(n1)], (b, j, delta)
            assert dg[b] == sums(now[b]) and dg[b][0] != seal[b][0]
            # the residue identity holds on the wrong operand: the words are the checked inner sum's on the corrupted row, no flag there
            c0, c1, cf0, cf1 = inner_checked(checked, now, y0, y1, q, path)
            assert fl == [0, 0] == [cf0, cf1] and (w0 == c0).all() and (w1 == c1).all()
            assert w0.tolist() == dot(now, y0, q)
        # two words of one row, among them d1 = -d2 (S0 does not move, S1 does) at a distance that is a multiple of 3 * 5 * 17
        for b, j1, j2, d1, d2 in ((0, 0, n - 1, 5, -5), (n1 - 1, 1, 1 + 255 if n > 256 else 16, 1 << 10, -(1 << 10)), (n1 // 2, 3, 4, 9, 2),
                                  (0, n // 2, n // 2 + 1, -1, 1)):
            now = d.copy()
            now[b][j1] = int(d[b][j1]) + d1
            now[b][j2] = int(d[b][j2]) + d2
            assert (now < np.uint64(q)).all()
            if d1 + d2 == 0:
                assert sums(now[b])[0] == seal[b][0] and sums(now[b])[1] != seal[b][1]
            sf = sealed(emu, now, y0, y1, q, path, log_chunk, seal)[4]
            assert sf == [SUM if r == b else 0 for r in range(n1)], (b, j1, j2, d1, d2)


@pytest.mark.parametrize("path,bits", PATHS)
def test_a_word_plus_k_p_outside_the_window_raises_the_range_bit(emu, checked, path, bits):
    n, log_chunk, n1 = 1 << 13, 10, 5
    q = PRIMES[bits, n]
    d, y0, y1 = operands(np.random.default_rng(bits), q, n1, n)
    seal = seals(d)
    # x + k p is invisible to both sums; p > q, so it always lands outside the window, and x + 7 p < 2^64
    for b, j, k in ((0, 0, 1), (n1 - 1, n - 1, 7), (2, (1 << 10) + 1, 3)):
        now = d.copy()
        v = int(d[b][j]) + k * P
        assert q <= v < 1 << 64
        now[b][j] = v
        assert sums(now[b]) == seal[b]
        w0, w1, fl, dg, sf = sealed(emu, now, y0, y1, q, path, log_chunk, seal)
        assert sf == [RANGE if r == b else 0 for r in range(n1)], (b, j, k)
        # the residue check cannot cover it: bit 4 on both parts, the words still the unchecked kernel's
        c0, c1, cf0, cf1 = inner_checked(checked, now, y0, y1, q, path)
        assert fl == [OPERAND, OPERAND] == [cf0, cf1] and (w0 == c0).all() and (w1 == c1).all()
        assert w0.tolist() == dot(now, y0, q) and w1.tolist() == dot(now, y1, q)
    # a single-bit flip that leaves the window moves the sums as well: q never divides 2^b
    now = d.copy()
    now[1][9] = int(d[1][9]) | (1 << 62)
    assert sealed(emu, now, y0, y1, q, path, log_chunk, seal)[4] == [0, SUM | RANGE, 0, 0, 0]


def test_a_stored_seal_that_is_not_canonical_counts_as_moved(emu):
    n, log_chunk, n1 = 1 << 5, 5, 4
    q = PRIMES[50, n]
    d, y0, y1 = operands(np.random.default_rng(1), q, n1, n)
    d[2][:] = 0                                          # both sums of this row are 0, and p stands for 0 modulo p
    seal = seals(d)
    assert seal[2] == [0, 0]
    assert sealed(emu, d, y0, y1, q, "u64", log_chunk, seal)[4] == [0, 0, 0, 0]
    for i in (0, 1):
        bad = [list(s) for s in seal]
        bad[2][i] = P
        assert sealed(emu, d, y0, y1, q, "u64", log_chunk, bad)[4] == [0, 0, SUM, 0], i
    # a canonical sum plus p, where that fits 64 bits
    bad = [list(s) for s in seal]
    bad[0][0] += P
    assert bad[0][0] < 1 << 64
    assert sealed(emu, d, y0, y1, q, "u64", log_chunk, bad)[4] == [SUM, 0, 0, 0]


@pytest.mark.parametrize("path,bits", PATHS)
def test_a_flip_on_the_consuming_load_raises_its_row_and_not_the_residue_check(emu, checked, path, bits):
    for (n, log_chunk), n1 in zip(CUTS, (1, 16, 4, 5)):
        q = PRIMES[bits, n]
        d, y0, y1 = operands(np.random.default_rng(bits + n1), q, n1, n)
        d = np.minimum(d, np.uint64(q - 17)) | np.uint64(1 << 3)      # bit 3 is set in every word: the flipped word stays below q
        assert (d < np.uint64(q)).all()
        seal = seals(d)
        for b, j in ((0, 0), (n1 - 1, n - 1), (n1 // 2, n // 2 + 1)):
            w0, w1, fl, dg, sf = sealed(emu, d, y0, y1, q, path, log_chunk, seal, hit=(b, j, 3))
            now = d.copy()
            now[b][j] = int(d[b][j]) ^ (1 << 3)
            assert sf == [SUM if r == b else 0 for r in range(n1)] and fl == [0, 0], (b, j)
            assert dg == seals(now)
            assert w0.tolist() == dot(now, y0, q) and w1.tolist() == dot(now, y1, q)
        # the hook is a function of the armed word alone: none armed, nothing raised
        assert sealed(emu, d, y0, y1, q, path, log_chunk, seal)[4] == [0] * n1
