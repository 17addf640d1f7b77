"""CPU emulation of the row seals (tests/emu/emu_seal_check.cpp compiles seal_check.hpp, the functions the kernels of
seal_checked.hip call): seals equal Python-integer sums modulo p = 2^61 - 1, do not depend on how a row is cut into chunks, and
every change confined to one or two words of a row is caught -- without a GPU.

The changes a fold modulo 2^32 - 1 cannot see are constructed on purpose and none is filtered out: +-(2^b - 2^(b+32)) inside one
word (asserted here to pass residue_check.hpp's fold unseen), and d1 = -d2 on two words whose distance is a multiple of 3 * 5 * 17."""
import ctypes as C

import numpy as np
import pytest

from helpers.emu_build import build_emu
from oracle import cport as O

p64 = C.POINTER(C.c_uint64)
p32 = C.POINTER(C.c_uint32)
P = (1 << 61) - 1
SUM, RANGE = 1, 2
BITS = [30, 50, 61]
SIZES = [1 << 5, 1 << 13]
PRIMES = {(bits, n): O.gen_primes(n, bits, 1)[0] for bits in BITS for n in SIZES}


@pytest.fixture(scope="module")
def emu():
    L = build_emu("libemu_seal_check.so", ["emu_seal_check.cpp"], ("modarith.hpp", "residue_check.hpp", "seal_check.hpp"))
    L.emu_seal.restype = None
    L.emu_seal.argtypes = [p64, C.c_size_t, C.c_size_t, p64]
    L.emu_seal_chunked.restype = None
    L.emu_seal_chunked.argtypes = [p64, C.c_size_t, C.c_size_t, C.c_int, p64]
    L.emu_seal_verify.restype = None
    L.emu_seal_verify.argtypes = [p64, C.c_size_t, C.c_size_t, C.c_uint64, p64, p32]
    L.emu_seal_canonical.restype = C.c_uint64
    L.emu_seal_canonical.argtypes = [C.c_uint64]
    L.emu_fold32_equal.restype = C.c_int
    L.emu_fold32_equal.argtypes = [C.c_uint64, C.c_uint64]
    return L


def _p(a):
    return a.ctypes.data_as(p64)


def seal(emu, x, log_chunk=None):
    x = np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, np.shape(x)[-1])
    out = np.zeros((x.shape[0], 2), dtype=np.uint64)
    if log_chunk is None:
        emu.emu_seal(_p(x), x.shape[0], x.shape[1], _p(out))
    else:
        emu.emu_seal_chunked(_p(x), x.shape[0], x.shape[1], log_chunk, _p(out))
    return out


def verify(emu, x, q, s):
    x = np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, np.shape(x)[-1])
    s = np.ascontiguousarray(s, dtype=np.uint64)
    f = np.zeros(x.shape[0], dtype=np.uint32)
    emu.emu_seal_verify(_p(x), x.shape[0], x.shape[1], q, _p(s), f.ctypes.data_as(p32))
    return f


def want(x):
    """Python integers"""
    return [[sum(int(v) for v in row) % P, sum((j + 1) * int(v) for j, v in enumerate(row)) % P] for row in np.atleast_2d(x)]


def _row_with_s0_equal_p(q, n):
    """canonical words whose plain sum is exactly p, where n words below q can reach it; else None"""
    if n * (q - 1) < P:
        return None
    row, left = np.zeros(n, dtype=np.uint64), P
    for j in range(n):
        row[j] = min(q - 1, left)
        left -= int(row[j])
    assert left == 0 and sum(int(v) for v in row) == P and (row < np.uint64(q)).all()
    return row


def _rows(rng, q, n):
    rows = [rng.integers(0, q, n, dtype=np.uint64) for _ in range(3)]
    rows.append(np.full(n, q - 1, dtype=np.uint64))
    rows.append(np.zeros(n, dtype=np.uint64))
    return np.stack(rows)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bits", BITS)
def test_seals_equal_python_sums(emu, bits, n):
    q = PRIMES[bits, n]
    x = _rows(np.random.default_rng(bits + n), q, n)
    got = seal(emu, x)
    assert got.tolist() == want(x)
    assert (got < np.uint64(P)).all()
    assert not verify(emu, x, q, got).any()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bits", BITS)
def test_a_sum_that_lands_on_p_is_zero(emu, bits, n):
    q = PRIMES[bits, n]
    assert emu.emu_seal_canonical(P) == 0 and emu.emu_seal_canonical(2 * P) == 0 and emu.emu_seal_canonical(P - 1) == P - 1
    assert emu.emu_seal_canonical(2**64 - 1) == (2**64 - 1) % P
    # a seal takes any 64-bit words: the word p at index 0 (weight 1) puts BOTH sums on exactly p
    row = np.zeros(n, dtype=np.uint64)
    row[0] = P
    assert seal(emu, row).tolist() == [[0, 0]] == want(row)
    # canonical words, wherever n words below q can sum to p (not 30-bit primes, nor 50-bit ones at 2^5: the sum stays below p)
    row = _row_with_s0_equal_p(q, n)
    assert (row is not None) == (bits == 61 or (bits == 50 and n == 1 << 13))
    if row is not None:
        got = seal(emu, row)
        assert got[0, 0] == 0 and got.tolist() == want(row)
        assert not verify(emu, row, q, got).any()
        for lc in (5, 8, 11):
            if (1 << lc) <= n:
                assert seal(emu, row, lc).tolist() == got.tolist()


@pytest.mark.parametrize("bits", BITS)
def test_the_seal_does_not_depend_on_the_chunk_size(emu, bits):
    """partials of chunks of 2^5, 2^8 and 2^11 words, each summed as a workgroup sums it: the weight is the index in the row"""
    n = 1 << 13
    q = PRIMES[bits, n]
    x = _rows(np.random.default_rng(bits), q, n)
    x[0, ::7] = np.random.default_rng(1).integers(0, 2**64 - 1, x[0, ::7].size, dtype=np.uint64, endpoint=True)      # any 64-bit words
    one = seal(emu, x)
    assert one.tolist() == want(x)
    for lc in (5, 8, 11):
        assert seal(emu, x, lc).tolist() == one.tolist(), lc
    small = _rows(np.random.default_rng(bits + 1), PRIMES[bits, 32], 32)
    assert seal(emu, small, 5).tolist() == seal(emu, small).tolist() == want(small)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bits", BITS)
def test_every_one_word_change_is_caught(emu, bits, n):
    q = PRIMES[bits, n]
    rng = np.random.default_rng(3 * bits + n)
    x = rng.integers(0, q, n, dtype=np.uint64)
    s = seal(emu, x)
    for j in (0, 1, n // 2 + 3, n - 1):
        for bit in range(64):
            y = x.copy()
            y[j] ^= np.uint64(1 << bit)
            f = int(verify(emu, y, q, s)[0])
            assert f & SUM, (j, bit)      # 0 < |d| = 2^bit < 2^64, and 2^bit is never 0 modulo p
            assert bool(f & RANGE) == (int(y[j]) >= q), (j, bit)
    # the multi-bit change inside one word that the fold modulo 2^32 - 1 misses: +2^b - 2^(b+32) and its negative, as a pair of
    # bit flips (bit b clear and bit b + 32 set before for +, the other way round for -).  The seal is taken of the row as it is
    # before the change, whatever the forced bits made of that word
    seen_in_window = 0
    for b in range(32):
        for sign in (1, -1):
            j = (5 * b + 1) % n
            lo, hi = 1 << b, 1 << (b + 32)
            before = (int(x[j]) & ~lo) | hi if sign > 0 else (int(x[j]) | lo) & ~hi
            after = before + sign * (lo - hi)
            assert 0 <= after < 2**64 and bin(before ^ after).count("1") == 2
            y = x.copy()
            y[j] = before
            s_y = seal(emu, y)
            y[j] = after
            assert emu.emu_fold32_equal(before, after) == 1, (b, sign)      # residue_check.hpp's fold does not see it
            f = int(verify(emu, y, q, s_y)[0])
            assert f & SUM, (b, sign)      # d = +-(2^b - 2^(b+32)) is not 0 modulo p
            assert bool(f & RANGE) == (after >= q), (b, sign)
            seen_in_window += after < q
    if bits == 61:
        assert seen_in_window >= 25      # on 61-bit words most of these stay below q: only the sums see them


@pytest.mark.parametrize("bits", BITS)
def test_two_word_changes_are_caught(emu, bits):
    n = 1 << 13
    q = PRIMES[bits, n]
    rng = np.random.default_rng(bits)
    x = rng.integers(q // 4, q - q // 4, n, dtype=np.uint64)
    s = seal(emu, x)
    step = 3 * 5 * 17
    checked = 0
    for j1 in (0, 1, 77):
        for dist in range(step, n - j1, step):      # EVERY multiple of 255 that fits
            j2 = j1 + dist
            for d in (1, 2**32 - 1 if q > 2**36 else 3 * 5 * 17 * 257, q // 5):      # each keeps both words inside [0, q)
                y = x.copy()
                y[j1] = int(x[j1]) + d
                y[j2] = int(x[j2]) - d
                assert 0 <= int(y[j1]) < q and 0 <= int(y[j2]) < q
                got = seal(emu, y)
                assert got[0, 0] == s[0, 0] and got[0, 1] != s[0, 1], (j1, j2, d)      # S0 cannot see it, S1 must
                assert int(verify(emu, y, q, s)[0]) == SUM, (j1, j2, d)
                checked += 1
    assert checked == 3 * sum(len(range(step, n - j1, step)) for j1 in (0, 1, 77))
    # a word raised to q, and to q with the other word lowered so that S0 holds
    k, j = np.argsort(x)[-2:]      # the two largest words: x[k] >= q - x[j]
    y = x.copy()
    y[j] = q
    assert int(verify(emu, y, q, s)[0]) == SUM | RANGE
    y[k] = int(x[k]) - (q - int(x[j]))
    assert seal(emu, y)[0, 0] == s[0, 0] and int(verify(emu, y, q, s)[0]) == SUM | RANGE
    # N = 2^5: every pair of positions
    n = 1 << 5
    q = PRIMES[bits, n]
    x = rng.integers(q // 4, q - q // 4, n, dtype=np.uint64)
    s = seal(emu, x)
    for j1 in range(n):
        for j2 in range(j1 + 1, n):
            y = x.copy()
            y[j1] += np.uint64(12345)
            y[j2] -= np.uint64(12345)
            assert int(verify(emu, y, q, s)[0]) == SUM
