"""CPU emulation of the checked inner sum of the BSGS product and of the checked add (tests/emu/emu_bsgs_check.cpp compiles
bsgs_check.hpp, the element functions the kernels of bsgs_checked.hip call): clean words equal Python-integer results, the two
ciphertext parts are independent, and a bit flip at any injection point raises a flag exactly when it changes the output word --
without a GPU."""
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
# the running sums are folded after every eighth term: 0, 0, 0, 1, 1, 2, 2 and 8 folds
N1S = [1, 2, 7, 8, 9, 16, 17, 64]
# (path, bits): the U64 form serves every limb, the FP64-term form only limbs below 2^50
PATHS = [("u64", 30), ("u64", 50), ("u64", 61), ("f64", 30), ("f64", 50)]


@pytest.fixture(scope="module")
def emu():
    L = build_emu("libemu_bsgs_check.so", ["emu_bsgs_check.cpp"], ("modarith.hpp", "residue_check.hpp", "baseconv_check.hpp", "keyswitch_check.hpp",
                                                                   "bsgs_check.hpp"))
    L.emu_diag_mac_checked.restype = C.c_int
    L.emu_diag_mac_checked.argtypes = [p64, p64, p64, C.c_int, C.c_size_t, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, p64, p64, p32, p32]
    L.emu_diag_mac_plain.restype = C.c_int
    L.emu_diag_mac_plain.argtypes = [p64, p64, p64, C.c_int, C.c_size_t, C.c_uint64, C.c_int, p64, p64]
    L.emu_modadd_checked.restype = C.c_int
    L.emu_modadd_checked.argtypes = [p64, p64, C.c_size_t, C.c_uint64, C.c_int, C.c_int, p64, p32]
    L.emu_modadd_plain.restype = C.c_int
    L.emu_modadd_plain.argtypes = [p64, p64, C.c_size_t, C.c_uint64, p64]
    return L


def _u(x):
    return np.ascontiguousarray(x, dtype=np.uint64)


def _p(a):
    return a.ctypes.data_as(p64)


def _f(a):
    return a.ctypes.data_as(p32)


def inner(emu, d, y0, y1, q, path, half=0, point=-1, bit=0):
    """d, y0, y1: [n1][n]; returns (w0, w1, f0, f1); the flip hits part `half`."""
    d, y0, y1 = _u(d), _u(y0), _u(y1)
    n = d.shape[1]
    w0, w1 = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    f0, f1 = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    assert emu.emu_diag_mac_checked(_p(d), _p(y0), _p(y1), d.shape[0], n, q, 0 if path == "f64" else 1, half, point, bit, _p(w0), _p(w1), _f(f0), _f(f1)) == 0
    return w0, w1, f0, f1


def add(emu, a, b, q, point=-1, bit=0):
    a, b = _u(a), _u(b)
    w, f = np.zeros(a.size, dtype=np.uint64), np.zeros(a.size, dtype=np.uint32)
    assert emu.emu_modadd_checked(_p(a), _p(b), a.size, q, point, bit, _p(w), _f(f)) == 0
    return w, f


def _rand(rng, q, shape):
    return rng.integers(0, q, shape, dtype=np.uint64)


def _dot_want(x, y, q):
    return [sum((int(x[t, i]) % q) * (int(y[t, i]) % q) for t in range(x.shape[0])) % q for i in range(x.shape[1])]


@pytest.mark.parametrize("path,bits", PATHS)
@pytest.mark.parametrize("n1", N1S)
def test_inner_sum_clean_words_are_exact_and_raise_nothing(emu, path, bits, n1):
    q = PRIMES[bits]
    rng = np.random.default_rng(bits + 131 * n1)
    d, y0, y1 = (_rand(rng, q, (n1, 400)) for _ in range(3))
    # edge operands: 0, 1 and q - 1 in every term; q - 1 against q - 1 everywhere makes the largest sum
    for v, at in ((0, 0), (1, 1), (q - 1, 2)):
        d[:, at] = v
        y0[:, at] = v
        y1[:, at] = v
    w0, w1, f0, f1 = inner(emu, d, y0, y1, q, path)
    assert [int(v) for v in w0] == _dot_want(d, y0, q)
    assert [int(v) for v in w1] == _dot_want(d, y1, q)
    assert not f0.any() and not f1.any()
    # the two parts are independent: another part 1 leaves part 0's words alone
    v0, v1, g0, g1 = inner(emu, d, y0, _rand(rng, q, (n1, 400)), q, path)
    assert (v0 == w0).all() and (v1 != w1).any() and not g0.any() and not g1.any()


@pytest.mark.parametrize("path,bits", PATHS)
@pytest.mark.parametrize("n1", N1S)
def test_inner_sum_flip_is_flagged_exactly_when_it_changes_the_word(emu, path, bits, n1):
    q = PRIMES[bits]
    rng = np.random.default_rng(1000 + bits + 131 * n1)
    d, y0, y1 = (_rand(rng, q, (n1, 64)) for _ in range(3))
    clean = inner(emu, d, y0, y1, q, path)
    assert not clean[2].any() and not clean[3].any()
    assert [int(v) for v in clean[0]] == _dot_want(d, y0, q) and [int(v) for v in clean[1]] == _dot_want(d, y1, q)
    for half in (0, 1):
        for point in (PRODUCT, QUOTIENT, RESULT, SUM):
            flagged_bits, flagged_and_changed = 0, 0
            for bit in range(64):
                got = inner(emu, d, y0, y1, q, path, half, point, bit)
                w, f = got[half], got[2 + half]
                changed, flagged = w != clean[half], f != 0
                bad = np.nonzero(changed != flagged)[0]
                assert bad.size == 0, f"part {half} point {point} bit {bit}: element {bad[0]} word {clean[half][bad[0]]} -> {w[bad[0]]}, flags {f[bad[0]]}"
                assert not (f & OPERAND).any()
                # the other part: same words, no flag
                assert (got[1 - half] == clean[1 - half]).all() and not got[3 - half].any(), f"part {half} point {point} bit {bit} reached the other part"
                flagged_bits += int(flagged.any())
                flagged_and_changed += int((flagged & changed).any())
                if point == RESULT:
                    assert flagged.all() and changed.all(), f"bit {bit} of the result word not caught"
            assert flagged_bits >= 1 and flagged_and_changed >= 1, f"part {half} point {point}: no flip was flagged"
            if point == RESULT:
                assert flagged_bits == 64


@pytest.mark.parametrize("path,bits", PATHS)
@pytest.mark.parametrize("n1", [1, 8, 9, 17])
def test_inner_sum_noncanonical_words_raise_bit_4_and_keep_the_unchecked_word(emu, path, bits, n1):
    q = PRIMES[bits]
    rng = np.random.default_rng(bits + n1)
    n = 96
    d, y0, y1 = (_rand(rng, q, (n1, n)) for _ in range(3))
    big = rng.integers(q, 2**64 - 1, n, dtype=np.uint64, endpoint=True)
    d[0, ::4] = big[::4]                       # a diagonal word out of range: both parts
    y0[n1 - 1, 1::4] = big[1::4]               # a word of part 0 only
    y1[n1 // 2, 2::4] = q                      # exactly q, part 1 only
    bad_d = (d >= q).any(axis=0)
    bad0, bad1 = bad_d | (y0 >= q).any(axis=0), bad_d | (y1 >= q).any(axis=0)
    assert bad0.any() and (~bad0).any() and (bad0 != bad1).any()
    w0, w1, f0, f1 = inner(emu, d, y0, y1, q, path)
    p0, p1 = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    assert emu.emu_diag_mac_plain(_p(d), _p(y0), _p(y1), n1, n, q, 0 if path == "f64" else 1, _p(p0), _p(p1)) == 0
    assert (w0 == p0).all() and (w1 == p1).all()
    assert [int(v) for v in w0] == _dot_want(d, y0, q) and [int(v) for v in w1] == _dot_want(d, y1, q)
    assert (f0[bad0] == OPERAND).all() and not f0[~bad0].any()
    assert (f1[bad1] == OPERAND).all() and not f1[~bad1].any()


def _add_ops(rng, q, n):
    a, b = _rand(rng, q, n), _rand(rng, q, n)
    # the edge words 0, 1, q - 1 on both sides and a + b = q exactly
    edges = [(0, 0), (0, 1), (1, 1), (0, q - 1), (q - 1, 0), (1, q - 1), (q - 1, q - 1), (q - 1, 1), (q // 2, q - q // 2), (5, q - 5)]
    for i, (x, y) in enumerate(edges):
        a[i], b[i] = x, y
    return a, b


@pytest.mark.parametrize("bits", [30, 50, 61])
def test_add_clean_words_are_exact_and_raise_nothing(emu, bits):
    q = PRIMES[bits]
    a, b = _add_ops(np.random.default_rng(bits), q, 4000)
    assert ((a.astype(object) + b.astype(object)) == q).any()
    w, f = add(emu, a, b, q)
    assert [int(v) for v in w] == [(int(x) + int(y)) % q for x, y in zip(a, b)]
    assert not f.any()


@pytest.mark.parametrize("bits", [30, 50, 61])
def test_add_flip_is_flagged_exactly_when_it_changes_the_word(emu, bits):
    q = PRIMES[bits]
    a, b = _add_ops(np.random.default_rng(77 + bits), q, 200)
    clean, f0 = add(emu, a, b, q)
    assert not f0.any()
    for point in (RESULT, SUM):
        for bit in range(64):
            w, f = add(emu, a, b, q, point, bit)
            changed, flagged = w != clean, f != 0
            bad = np.nonzero(changed != flagged)[0]
            assert bad.size == 0, f"point {point} bit {bit}: element {bad[0]} word {clean[bad[0]]} -> {w[bad[0]]}, flags {f[bad[0]]}"
            assert not (f & OPERAND).any()
            # a flip of the word or of a + b always changes the word (2^j is no multiple of q): every bit is caught on every element
            assert flagged.all() and changed.all(), f"point {point} bit {bit} not caught"
    # there is no product and no quotient estimate on an add
    w, f = np.zeros(a.size, dtype=np.uint64), np.zeros(a.size, dtype=np.uint32)
    for point in (PRODUCT, QUOTIENT):
        assert emu.emu_modadd_checked(_p(a), _p(b), a.size, q, point, 0, _p(w), _f(f)) != 0


@pytest.mark.parametrize("bits", [30, 50, 61])
def test_add_noncanonical_operands_raise_bit_4_and_keep_the_plain_word(emu, bits):
    q = PRIMES[bits]
    rng = np.random.default_rng(bits + 9)
    n = 96
    a, b = _rand(rng, q, n), _rand(rng, q, n)
    big = rng.integers(q, 2**64 - 1, n, dtype=np.uint64, endpoint=True)
    a[::4] = big[::4]
    b[1::4] = big[1::4]
    b[3::8] = q
    bad = (a >= q) | (b >= q)
    assert bad.any() and (~bad).any()
    w, f = add(emu, a, b, q)
    plain = np.zeros(n, dtype=np.uint64)
    assert emu.emu_modadd_plain(_p(a), _p(b), n, q, _p(plain)) == 0
    assert (w == plain).all()
    assert [int(v) for v in w] == [(int(x) % q + int(y) % q) % q for x, y in zip(a, b)]
    assert (f[bad] == OPERAND).all() and not f[~bad].any()
