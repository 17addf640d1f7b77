"""CPU emulation of the checked key-switch inner product and mod-down tail (tests/emu/emu_keyswitch_check.cpp compiles
keyswitch_check.hpp, the element functions the kernels of keyswitch_checked.hip call): clean words equal Python-integer
results, and a bit flip at any injection point raises a flag exactly when it changes the output word -- without a GPU."""
import ctypes as C

import numpy as np
import pytest

from helpers.emu_build import build_emu
from oracle import cport as O

p64 = C.POINTER(C.c_uint64)
p32 = C.POINTER(C.c_uint32)
RESIDUE, RANGE, OPERAND = 1, 2, 4
PRODUCT, QUOTIENT, RESULT, SUM = 0, 1, 2, 3
N = 1 << 16
PRIMES = {bits: O.gen_primes(N, bits, 1)[0] for bits in (30, 50, 61)}
# every value crosses a different number of folds of the running sum (one after every eighth term)
DNUMS = [1, 4, 7, 8, 9, 11, 16, 17, 44, 64]
# (path, bits): the U64 form serves every limb, the FP64-term form only limbs below 2^50
PATHS = [("u64", 30), ("u64", 50), ("u64", 61), ("f64", 30), ("f64", 50)]


@pytest.fixture(scope="module")
def emu():
    L = build_emu("libemu_keyswitch_check.so", ["emu_keyswitch_check.cpp"], ("modarith.hpp", "residue_check.hpp", "baseconv_check.hpp",
                                                                             "keyswitch_check.hpp"))
    L.emu_ks_dot_checked.restype = C.c_int
    L.emu_ks_dot_checked.argtypes = [p64, p64, C.c_int, C.c_size_t, C.c_uint64, C.c_int, C.c_int, C.c_int, p64, p32]
    L.emu_ks_dot_plain.restype = C.c_int
    L.emu_ks_dot_plain.argtypes = [p64, p64, C.c_int, C.c_size_t, C.c_uint64, C.c_int, p64]
    L.emu_ks_tail_checked.restype = C.c_int
    L.emu_ks_tail_checked.argtypes = [p64, p64, p64, C.c_int, C.c_size_t, C.c_uint64, C.c_uint64, C.c_int, C.c_int, p64, p32]
    L.emu_ks_tail_plain.restype = C.c_int
    L.emu_ks_tail_plain.argtypes = [p64, p64, p64, C.c_int, C.c_size_t, C.c_uint64, C.c_uint64, p64]
    return L


def _u(x):
    return np.ascontiguousarray(x, dtype=np.uint64)


def _p(a):
    return a.ctypes.data_as(p64)


def dot(emu, x, y, q, path, point=-1, bit=0):
    """x, y: [terms][n]; path "f64" = FP64-term form, "u64" = Barrett form."""
    x, y = _u(x), _u(y)
    n = x.shape[1]
    w, f = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
    assert emu.emu_ks_dot_checked(_p(x), _p(y), x.shape[0], n, q, 0 if path == "f64" else 1, point, bit, _p(w), f.ctypes.data_as(p32)) == 0
    return w, f


def tail(emu, x, y, add, q, s, point=-1, bit=0):
    x, y = _u(x), _u(y)
    a = _u(add) if add is not None else np.zeros(1, dtype=np.uint64)
    w, f = np.zeros(x.size, dtype=np.uint64), np.zeros(x.size, dtype=np.uint32)
    assert emu.emu_ks_tail_checked(_p(x), _p(y), _p(a), int(add is not None), x.size, q, s, point, bit, _p(w), f.ctypes.data_as(p32)) == 0
    return w, f


def _rand(rng, q, shape):
    return rng.integers(0, q, shape, dtype=np.uint64)


def _dot_want(x, y, q):
    return [sum(int(x[t, i]) * int(y[t, i]) for t in range(x.shape[0])) % q for i in range(x.shape[1])]


def _tail_want(x, y, add, q, s):
    return [((int(x[i]) - int(y[i])) * s + (int(add[i]) if add is not None else 0)) % q for i in range(x.size)]


def _check_flips(run, clean, points):
    """For every point and every bit 0-63: flagged exactly when the word changed; RESULT: all 64 bits flagged; every other point:
    some bit flagged, and some flagged bit changed the word."""
    for point in points:
        flagged_bits, flagged_and_changed = 0, 0
        for bit in range(64):
            w, f = run(point, bit)
            changed, flagged = w != clean, f != 0
            bad = np.nonzero(changed != flagged)[0]
            assert bad.size == 0, f"point {point} bit {bit}: element {bad[0]} word {clean[bad[0]]} -> {w[bad[0]]}, flags {f[bad[0]]}"
            assert not (f & OPERAND).any()
            flagged_bits += int(flagged.any())
            flagged_and_changed += int((flagged & changed).any())
            if point == RESULT:
                assert flagged.all() and changed.all(), f"bit {bit} of the result word not caught"
        assert flagged_bits >= 1 and flagged_and_changed >= 1, f"point {point}: no flip was flagged"
        if point == RESULT:
            assert flagged_bits == 64


@pytest.mark.parametrize("path,bits", PATHS)
@pytest.mark.parametrize("dnum", DNUMS)
def test_inner_product_clean_words_are_exact_and_raise_nothing(emu, path, bits, dnum):
    q = PRIMES[bits]
    rng = np.random.default_rng(bits + 131 * dnum)
    x, y = _rand(rng, q, (dnum, 600)), _rand(rng, q, (dnum, 600))
    # edge operands: 0, 1 and q - 1 in every term; q - 1 against q - 1 everywhere makes the largest sum
    for v, at in ((0, 0), (1, 1), (q - 1, 2)):
        x[:, at] = v
        y[:, at] = v
    w, f = dot(emu, x, y, q, path)
    assert [int(v) for v in w] == _dot_want(x, y, q)
    assert not f.any()


@pytest.mark.parametrize("path,bits", PATHS)
@pytest.mark.parametrize("dnum", DNUMS)
def test_inner_product_flip_is_flagged_exactly_when_it_changes_the_word(emu, path, bits, dnum):
    q = PRIMES[bits]
    rng = np.random.default_rng(1000 + bits + 131 * dnum)
    x, y = _rand(rng, q, (dnum, 120)), _rand(rng, q, (dnum, 120))
    clean, f0 = dot(emu, x, y, q, path)
    assert not f0.any() and [int(v) for v in clean] == _dot_want(x, y, q)
    _check_flips(lambda point, bit: dot(emu, x, y, q, path, point, bit), clean, [PRODUCT, QUOTIENT, RESULT, SUM])


@pytest.mark.parametrize("path,bits", PATHS)
@pytest.mark.parametrize("dnum", [1, 8, 11, 44])
def test_inner_product_noncanonical_operands_raise_bit_4_and_keep_the_unchecked_word(emu, path, bits, dnum):
    q = PRIMES[bits]
    rng = np.random.default_rng(bits + dnum)
    n = 96
    x, y = _rand(rng, q, (dnum, n)), _rand(rng, q, (dnum, n))
    big = rng.integers(q, 2**64 - 1, n, dtype=np.uint64, endpoint=True)
    x[0, ::3] = big[::3]                       # a digit word out of range (the digit's own limb of d_c)
    y[dnum - 1, 1::3] = big[1::3]              # a key word out of range
    x[dnum // 2, 5::12] = q                    # exactly q
    bad = (x >= q).any(axis=0) | (y >= q).any(axis=0)
    assert bad.any() and (~bad).any()
    w, f = dot(emu, x, y, q, path)
    plain = np.zeros(n, dtype=np.uint64)
    assert emu.emu_ks_dot_plain(_p(x), _p(y), dnum, n, q, 0 if path == "f64" else 1, _p(plain)) == 0
    assert (w == plain).all()
    assert [int(v) for v in w] == [sum((int(x[t, i]) % q) * (int(y[t, i]) % q) for t in range(dnum)) % q for i in range(n)]
    assert (f[bad] == OPERAND).all() and not f[~bad].any()


def _tail_ops(rng, q, n):
    x, y, add = _rand(rng, q, n), _rand(rng, q, n), _rand(rng, q, n)
    # x < y, x = y, and the edge words 0 and q - 1 in every position
    x[0], y[0] = 5, q - 3
    x[1], y[1] = 12345 % q, 12345 % q
    x[2], y[2], add[2] = 0, 0, 0
    x[3], y[3], add[3] = q - 1, 0, q - 1
    x[4], y[4], add[4] = 0, q - 1, q - 1
    x[5], y[5], add[5] = q - 1, q - 1, 0
    return x, y, add


@pytest.mark.parametrize("bits", [30, 50, 61])
@pytest.mark.parametrize("with_add", [False, True])
def test_tail_clean_words_are_exact_and_raise_nothing(emu, bits, with_add):
    q = PRIMES[bits]
    rng = np.random.default_rng(bits + 5 * with_add)
    x, y, add = _tail_ops(rng, q, 4000)
    assert (x < y).any() and (x == y).any() and (x > y).any()
    for s in (1, q - 1, int(rng.integers(2, q))):
        w, f = tail(emu, x, y, add if with_add else None, q, s)
        assert [int(v) for v in w] == _tail_want(x, y, add if with_add else None, q, s)
        assert not f.any()


@pytest.mark.parametrize("bits", [30, 50, 61])
@pytest.mark.parametrize("with_add", [False, True])
def test_tail_flip_is_flagged_exactly_when_it_changes_the_word(emu, bits, with_add):
    q = PRIMES[bits]
    rng = np.random.default_rng(77 + bits + 5 * with_add)
    x, y, add = _tail_ops(rng, q, 200)
    add = add if with_add else None
    s = int(rng.integers(2, q))
    clean, f0 = tail(emu, x, y, add, q, s)
    assert not f0.any() and [int(v) for v in clean] == _tail_want(x, y, add, q, s)
    # the running sum exists only with an addend
    points = [PRODUCT, QUOTIENT, RESULT] + ([SUM] if with_add else [])
    _check_flips(lambda point, bit: tail(emu, x, y, add, q, s, point, bit), clean, points)
    if not with_add:
        w, f = np.zeros(x.size, dtype=np.uint64), np.zeros(x.size, dtype=np.uint32)
        assert emu.emu_ks_tail_checked(_p(x), _p(y), _p(x), 0, x.size, q, s, SUM, 0, _p(w), f.ctypes.data_as(p32)) != 0


@pytest.mark.parametrize("bits", [30, 50, 61])
@pytest.mark.parametrize("with_add", [False, True])
def test_tail_noncanonical_operands_raise_bit_4_and_keep_the_unchecked_word(emu, bits, with_add):
    q = PRIMES[bits]
    rng = np.random.default_rng(bits + 9 * with_add)
    n = 96
    x, y, add = _rand(rng, q, n), _rand(rng, q, n), _rand(rng, q, n)
    big = rng.integers(q, 2**64 - 1, n, dtype=np.uint64, endpoint=True)
    x[::4] = big[::4]
    y[1::4] = big[1::4]
    y[3::8] = q
    if with_add:
        add[2::4] = big[2::4]
    bad = (x >= q) | (y >= q) | ((add >= q) if with_add else False)
    assert bad.any() and (~bad).any()
    s = int(rng.integers(2, q))
    w, f = tail(emu, x, y, add if with_add else None, q, s)
    plain = np.zeros(n, dtype=np.uint64)
    assert emu.emu_ks_tail_plain(_p(x), _p(y), _p(add), int(with_add), n, q, s, _p(plain)) == 0
    assert (w == plain).all()
    assert [int(v) for v in w] == _tail_want(x, y, add if with_add else None, q, s)
    assert (f[bad] == OPERAND).all() and not f[~bad].any()
