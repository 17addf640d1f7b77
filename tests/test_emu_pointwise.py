"""CPU emulation of the residue-checked element-wise products (tests/emu/emu_pointwise.cpp compiles residue_check.hpp, the
element functions the kernels of pointwise_checked.hip call): clean words equal Python-integer products, and a bit flip
at any injection point raises a flag exactly when it changes the output word -- without a GPU."""
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
# primes as create_moduli makes them (the oracle's restatement of CoeffModulus::Create)
PRIMES = {bits: O.gen_primes(N, bits, 1)[0] for bits in (30, 50, 61)}


@pytest.fixture(scope="module")
def emu():
    L = build_emu("libemu_pointwise.so", ["emu_pointwise.cpp"], ("modarith.hpp", "residue_check.hpp"))
    L.emu_modmul_checked.restype = C.c_int
    L.emu_modmul_checked.argtypes = [p64, p64, p64, C.c_size_t, C.c_uint64, C.c_int, C.c_int, C.c_int, p64, p32]
    L.emu_modmul_plain.restype = C.c_int
    L.emu_modmul_plain.argtypes = [p64, p64, p64, C.c_size_t, C.c_uint64, C.c_int, p64]
    L.emu_dot_checked.restype = C.c_int
    L.emu_dot_checked.argtypes = [p64, p64, C.c_int, C.c_size_t, C.c_uint64, C.c_int, C.c_int, C.c_int, p64, p32]
    return L


def _u(x):
    return np.ascontiguousarray(x, dtype=np.uint64)


def modmul(emu, a, b, o, q, acc, point=-1, bit=0):
    a, b, o = _u(a), _u(b), _u(o)
    w, f = np.zeros(a.size, dtype=np.uint64), np.zeros(a.size, dtype=np.uint32)
    assert emu.emu_modmul_checked(a.ctypes.data_as(p64), b.ctypes.data_as(p64), o.ctypes.data_as(p64), a.size, q, int(acc), point, bit,
                                  w.ctypes.data_as(p64), f.ctypes.data_as(p32)) == 0
    return w, f


def dot(emu, x, y, q, path, point=-1, bit=0):
    """x, y: [terms][n]; path 0 = FP64-term form, 1 = U64 (Barrett) form."""
    x, y = _u(x), _u(y)
    n = x.shape[1]
    w, f = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
    assert emu.emu_dot_checked(x.ctypes.data_as(p64), y.ctypes.data_as(p64), x.shape[0], n, q, path, point, bit, w.ctypes.data_as(p64),
                               f.ctypes.data_as(p32)) == 0
    return w, f


def _rand(rng, q, shape):
    return rng.integers(0, q, shape, dtype=np.uint64)


# (form, bits): the Barrett form serves every limb (k_modmul, KsMacU64); the FP64-term form only limbs below 2^50
FORMS = [("barrett", 30), ("barrett", 50), ("barrett", 61), ("u64", 30), ("u64", 50), ("u64", 61), ("f64", 30), ("f64", 50)]


def _run(emu, form, q, ops, acc, point=-1, bit=0):
    """ops = (a, b, o) for the Barrett form, (x [2][n], y [2][n]) for the sums; acc: with the old word / the two-term sum"""
    if form == "barrett":
        return modmul(emu, ops[0], ops[1], ops[2], q, acc, point, bit)
    terms = 2 if acc else 1
    return dot(emu, ops[0][:terms], ops[1][:terms], q, 0 if form == "f64" else 1, point, bit)


def _ops(rng, form, q, n):
    if form == "barrett":
        return _rand(rng, q, n), _rand(rng, q, n), _rand(rng, q, n)
    return _rand(rng, q, (2, n)), _rand(rng, q, (2, n))


def _want(form, q, ops, acc):
    if form == "barrett":
        a, b, o = ops
        return [((int(o[i]) if acc else 0) + int(a[i]) * int(b[i])) % q for i in range(a.size)]
    x, y = ops
    terms = 2 if acc else 1
    return [sum(int(x[t, i]) * int(y[t, i]) for t in range(terms)) % q for i in range(x.shape[1])]


@pytest.mark.parametrize("form,bits", FORMS)
@pytest.mark.parametrize("acc", [False, True])
def test_clean_words_are_exact_and_raise_nothing(emu, form, bits, acc):
    q = PRIMES[bits]
    rng = np.random.default_rng(bits + 7 * acc)
    ops = _ops(rng, form, q, 4000)
    # edge operands: 0, 1 and q - 1 everywhere
    for v, at in ((0, 0), (1, 1), (q - 1, 2)):
        for arr in ops:
            arr[..., at] = v
    w, f = _run(emu, form, q, ops, acc)
    assert [int(v) for v in w] == _want(form, q, ops, acc)
    assert not f.any()


# points that exist per form: the plain product has no running sum (point 3) to hit
def _points(form, acc):
    return [PRODUCT, QUOTIENT, RESULT] + ([SUM] if acc else [])


@pytest.mark.parametrize("form,bits", FORMS)
@pytest.mark.parametrize("acc", [False, True])
def test_a_flip_is_flagged_exactly_when_it_changes_the_word(emu, form, bits, acc):
    q = PRIMES[bits]
    rng = np.random.default_rng(1000 + bits + 7 * acc)
    ops = _ops(rng, form, q, 300)
    clean, f0 = _run(emu, form, q, ops, acc)
    assert not f0.any()
    unchanged_quiet = 0
    for point in _points(form, acc):
        for bit in range(64):
            w, f = _run(emu, form, q, ops, acc, point, bit)
            changed = w != clean
            flagged = f != 0
            bad = np.nonzero(changed != flagged)[0]
            assert bad.size == 0, (f"point {point} bit {bit}: element {bad[0]} word {clean[bad[0]]} -> {w[bad[0]]}, flags {f[bad[0]]}")
            assert not (f & OPERAND).any()
            if point != RESULT and point != PRODUCT:
                unchanged_quiet += int((~changed).sum())
    # A flip that leaves the word right is a consistent shift: the FP64 quotient of the final reduction moved by d with the
    # value moved by d q (or a fraction of the quotient too small to move the rounded word), or a Barrett quotient one
    # below its floor that the next conditional subtraction absorbs.  They exist, and (asserted above) raise nothing.
    if form == "f64":
        assert unchanged_quiet > 0


@pytest.mark.parametrize("form,bits", FORMS)
def test_every_single_flip_of_the_result_word_is_caught(emu, form, bits):
    # 2^j is never 0 mod 2^32 - 1: a flip of the stored word always changes it and is always flagged (residue, or window)
    q = PRIMES[bits]
    rng = np.random.default_rng(bits)
    ops = _ops(rng, form, q, 200)
    clean, _ = _run(emu, form, q, ops, True)
    for bit in range(64):
        w, f = _run(emu, form, q, ops, True, RESULT, bit)
        assert (w != clean).all() and (f != 0).all()
        if (1 << bit) < q:
            assert (f & RESIDUE).all()


@pytest.mark.parametrize("bits", [30, 50, 61])
@pytest.mark.parametrize("acc", [False, True])
def test_noncanonical_operands_raise_bit_4_and_keep_the_unchecked_word(emu, bits, acc):
    q = PRIMES[bits]
    rng = np.random.default_rng(bits + 3 * acc)
    n = 64
    a, b, o = _rand(rng, q, n), _rand(rng, q, n), _rand(rng, q, n)
    big = rng.integers(q, 2**64 - 1, n, dtype=np.uint64, endpoint=True)
    a[::4] = big[::4]                      # a out of range
    b[1::4] = big[1::4]                    # b out of range
    if acc:
        o[2::4] = big[2::4]                # the old word out of range
    a[3::8] = q                            # exactly q
    bad = (a >= q) | (b >= q) | ((o >= q) if acc else False)
    w, f = modmul(emu, a, b, o, q, acc)
    plain = np.zeros(n, dtype=np.uint64)
    assert emu.emu_modmul_plain(a.ctypes.data_as(p64), b.ctypes.data_as(p64), o.ctypes.data_as(p64), n, q, int(acc), plain.ctypes.data_as(p64)) == 0
    assert (w == plain).all()
    assert (f[bad] == OPERAND).all() and not f[~bad].any()
    # the sums reduce every operand first (KsMacF64 / KsMacU64): the word is the product of the reduced operands
    x, y = _rand(rng, q, (2, n)), _rand(rng, q, (2, n))
    x[0, ::3] = big[::3]
    y[1, 1::3] = big[1::3]
    bad = (x >= q).any(axis=0) | (y >= q).any(axis=0)
    for path in ([0, 1] if q < 2**50 else [1]):
        w, f = dot(emu, x, y, q, path)
        assert [int(v) for v in w] == [sum((int(x[t, i]) % q) * (int(y[t, i]) % q) for t in range(2)) % q for i in range(n)]
        assert (f[bad] == OPERAND).all() and not f[~bad].any()


def test_residue_arithmetic_folds_32_bit_halves(emu):
    # a flip of the quotient is a change of k by 2^j: r(k) r(q) moves by 2^j q, never 0 mod 2^32 - 1 for any odd q
    m = 2**32 - 1
    for q in PRIMES.values():
        assert all((pow(2, j, m) * q) % m for j in range(64))
    # the five primes that divide m still move by 2^j q: only a change of k by a multiple of m / q escapes the residue
    for q in (3, 5, 17, 257, 65537):
        assert m % q == 0 and all((pow(2, j, m) * q) % m for j in range(64))
