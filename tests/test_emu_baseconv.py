"""CPU emulation of the residue-checked base conversions (tests/emu/emu_baseconv.cpp compiles baseconv_check.hpp, the
element functions the kernels of baseconv_checked.hip call): clean digits and words equal Python-integer arithmetic, and a
bit flip at any injection point raises the flag of the unit it hit exactly when it changes that unit's digit / word --
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
SHAPES = [(1, 1), (3, 3), (8, 5), (11, 12), (16, 4), (20, 3)]
BITS = [30, 50, 61]
# 32 distinct primes per size, p = 1 mod 2^11 (the oracle's restatement of CoeffModulus::Create)
PRIMES = {bits: O.gen_primes(1 << 10, bits, 32) for bits in BITS}


def moduli(bits, m, k):
    """m input and k output primes of `bits` bits, all distinct"""
    return PRIMES[bits][:m], PRIMES[bits][m:m + k]


@pytest.fixture(scope="module")
def emu():
    L = build_emu("libemu_baseconv.so", ["emu_baseconv.cpp"], ("modarith.hpp", "residue_check.hpp", "baseconv_check.hpp"))
    L.emu_bc_exact_checked.restype = C.c_int
    L.emu_bc_exact_checked.argtypes = [p64, C.c_int, p64, C.c_int, p64, C.c_size_t, C.c_int, C.c_int, C.c_int, p64, p64, p32]
    L.emu_bc_exact_plain.restype = C.c_int
    L.emu_bc_exact_plain.argtypes = [p64, C.c_int, p64, C.c_int, p64, C.c_size_t, p64]
    L.emu_bc_fast_checked.restype = C.c_int
    L.emu_bc_fast_checked.argtypes = [p64, C.c_int, p64, C.c_int, p64, C.c_size_t, C.c_int, C.c_int, C.c_int, p64, p32]
    L.emu_bc_fast_plain.restype = C.c_int
    L.emu_bc_fast_plain.argtypes = [p64, C.c_int, p64, C.c_int, p64, C.c_size_t, p64]
    return L


def _u(x):
    return np.ascontiguousarray(x, dtype=np.uint64)


def _p(a, t=p64):
    return a.ctypes.data_as(t)


def exact(emu, mi, mo, x, point=-1, unit=0, bit=0, want_rc=0):
    """-> digits [m][n], words [k][n], flags [m + k][n]"""
    mi_, mo_, x = _u(mi), _u(mo), _u(x)
    m, n = x.shape
    d, w, f = np.zeros((m, n), np.uint64), np.zeros((len(mo), n), np.uint64), np.zeros((m + len(mo), n), np.uint32)
    rc = emu.emu_bc_exact_checked(_p(mi_), m, _p(mo_), len(mo), _p(x), n, point, unit, bit, _p(d), _p(w), _p(f, p32))
    assert rc == want_rc
    return d, w, f


def fast(emu, mi, mo, x, point=-1, unit=0, bit=0, want_rc=0):
    mi_, mo_, x = _u(mi), _u(mo), _u(x)
    m, n = x.shape
    w, f = np.zeros((len(mo), n), np.uint64), np.zeros((len(mo), n), np.uint32)
    rc = emu.emu_bc_fast_checked(_p(mi_), m, _p(mo_), len(mo), _p(x), n, point, unit, bit, _p(w), _p(f, p32))
    assert rc == want_rc
    return w, f


def rand_input(rng, mi, n):
    x = np.stack([rng.integers(0, p, n, dtype=np.uint64) for p in mi])
    # edge words in every limb: 0, 1, p_j - 1
    for j, p in enumerate(mi):
        x[j, 0], x[j, 1], x[j, 2] = 0, 1, p - 1
    return x


def py_exact(mi, mo, x):
    """mixed-radix digits and x mod q_o in Python integers (inputs reduced modulo p_j first)"""
    m, n = x.shape
    digits, words = np.zeros((m, n), np.uint64), np.zeros((len(mo), n), np.uint64)
    pref = [1]
    for p in mi:
        pref.append(pref[-1] * p)
    for i in range(n):
        val = 0
        for j, p in enumerate(mi):
            c = ((int(x[j, i]) - val) * pow(pref[j], -1, p)) % p
            digits[j, i] = c
            val += c * pref[j]
        for o, q in enumerate(mo):
            words[o, i] = val % q
    return digits, words


def py_fast(mi, mo, x):
    m, n = x.shape
    P = 1
    for p in mi:
        P *= p
    words = np.zeros((len(mo), n), np.uint64)
    for o, q in enumerate(mo):
        coef = [((P // p) % q) * pow((P // p) % p, -1, p) % q for p in mi]
        for i in range(n):
            words[o, i] = sum(int(x[j, i]) * coef[j] % q for j in range(m))
    return words


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("m,k", SHAPES)
def test_clean_digits_and_words_are_exact_and_raise_nothing(emu, bits, m, k):
    mi, mo = moduli(bits, m, k)
    x = rand_input(np.random.default_rng(bits * 100 + m), mi, 300)
    d, w, f = exact(emu, mi, mo, x)
    wd, ww = py_exact(mi, mo, x)
    assert (d == wd).all() and (w == ww).all()
    assert not f.any()
    if not fast_ok(m, mo):
        fast(emu, mi, mo, x, want_rc=-3)      # the unreduced sum would pass 64 bits: the fast call refuses such a plan
        return
    w, f = fast(emu, mi, mo, x)
    assert (w == py_fast(mi, mo, x)).all()
    assert not f.any()


def fast_ok(m, mo):
    return m * max(mo) < 2**64


def _points(terms):
    return [PRODUCT, QUOTIENT, RESULT] + ([SUM] if terms >= 2 else [])


# bits whose flip changes the value of every coefficient, by derivation: bit 0 of the low product word, of the running sum
# and of the result moves the value by 1; quotient bit 63 moves the remainder by 2^63 p = 2^63 (mod 2^64, p odd), which no
# multiple of p undoes (a quotient flip that leaves the word n p too high without wrapping is folded back and raises nothing)
SURE = {PRODUCT: 0, QUOTIENT: 63, RESULT: 0, SUM: 0}


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("m,k", [(4, 3), (20, 3)])
def test_exact_flip_is_flagged_on_its_unit_exactly_when_it_changes_the_value(emu, bits, m, k):
    mi, mo = moduli(bits, m, k)
    x = rand_input(np.random.default_rng(2000 + bits + m), mi, 200)
    d0, w0, f0 = exact(emu, mi, mo, x)
    assert not f0.any()
    clean = np.concatenate([d0, w0])
    for unit in (0, m // 2, m - 1, m + 1):          # first, a middle and the last digit, an output
        terms = unit + 1 if unit < m else m
        for point in _points(terms):
            for bit in range(64):
                d, w, f = exact(emu, mi, mo, x, point, unit, bit)
                changed = np.concatenate([d, w])[unit] != clean[unit]
                flagged = f[unit] != 0
                bad = np.nonzero(changed != flagged)[0]
                assert bad.size == 0, f"unit {unit} point {point} bit {bit}: coefficient {bad[0]} flags {f[unit, bad[0]]}"
                assert not (f & OPERAND).any()
                assert not np.delete(f, unit, axis=0).any(), f"unit {unit} point {point} bit {bit}: another unit is flagged"
                if bit == SURE[point]:
                    assert changed.all()
                if unit >= m:
                    assert (d == d0).all()
                elif bit <= 1:
                    # what the device test can observe: a digit is flagged exactly when an output word of the coefficient
                    # changes (a quotient 2^bit too low leaves the digit 2^bit p too high, which is folded back below 64 p
                    # and below 2^63; further out the digit is flagged on its window although the next digit would have
                    # compensated)
                    assert (flagged == (w != w0).any(axis=0)).all(), f"unit {unit} point {point} bit {bit}"
        # a point that does not exist there is refused
    exact(emu, mi, mo, x, SUM, 0, 0, want_rc=-2)


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("m,k", [(4, 3), (20, 3)])
def test_fast_flip_is_flagged_on_its_unit_exactly_when_it_changes_the_word(emu, bits, m, k):
    mi, mo = moduli(bits, m, k)
    if not fast_ok(m, mo):
        m = 7                                   # the longest base whose unreduced sum of 61-bit terms fits 64 bits
        mi = mi[:m]
    x = rand_input(np.random.default_rng(3000 + bits + m), mi, 200)
    w0, f0 = fast(emu, mi, mo, x)
    assert not f0.any()
    for unit in (0, k - 1):
        for point in _points(m):
            for bit in range(64):
                w, f = fast(emu, mi, mo, x, point, unit, bit)
                changed = w[unit] != w0[unit]
                bad = np.nonzero(changed != (f[unit] != 0))[0]
                assert bad.size == 0, f"unit {unit} point {point} bit {bit}: coefficient {bad[0]} flags {f[unit, bad[0]]}"
                assert not (f & OPERAND).any()
                assert not np.delete(f, unit, axis=0).any()
                assert (np.delete(w, unit, axis=0) == np.delete(w0, unit, axis=0)).all()
                if bit == SURE[point]:
                    assert changed.all()


def test_points_without_a_second_term_are_refused(emu):
    mi, mo = moduli(50, 1, 2)
    x = rand_input(np.random.default_rng(5), mi, 8)
    exact(emu, mi, mo, x, SUM, 0, 0, want_rc=-2)        # digit 0
    exact(emu, mi, mo, x, SUM, 1, 0, want_rc=-2)        # an output of a one-limb base
    fast(emu, mi, mo, x, SUM, 0, 0, want_rc=-2)
    exact(emu, mi, mo, x, PRODUCT, 3, 0, want_rc=-2)    # unit outside the call


@pytest.mark.parametrize("bits", BITS)
def test_every_single_flip_of_a_result_is_caught(emu, bits):
    # 2^j is never 0 mod 2^32 - 1: a flip of the digit / word always changes it and always fails the residue identity
    m, k = 5, 4
    mi, mo = moduli(bits, m, k)
    x = rand_input(np.random.default_rng(bits), mi, 200)
    d0, w0, _ = exact(emu, mi, mo, x)
    f0w, _ = fast(emu, mi, mo, x)
    for bit in range(64):
        for unit in (0, 2, m - 1, m, m + k - 1):
            d, w, f = exact(emu, mi, mo, x, RESULT, unit, bit)
            assert (np.concatenate([d, w])[unit] != np.concatenate([d0, w0])[unit]).all() and (f[unit] != 0).all()
            if (1 << bit) < (mi + mo)[unit]:
                assert (f[unit] & RESIDUE).all()
        w, f = fast(emu, mi, mo, x, RESULT, 1, bit)
        assert (w[1] != f0w[1]).all() and (f[1] != 0).all()
        if (1 << bit) < mo[1]:
            assert (f[1] & RESIDUE).all()


@pytest.mark.parametrize("bits", BITS)
def test_noncanonical_input_raises_bit_4_on_its_digit_and_keeps_the_unchecked_words(emu, bits):
    m, k, n = 6, 5, 96
    mi, mo = moduli(bits, m, k)
    rng = np.random.default_rng(bits + 11)
    x = rand_input(rng, mi, n)
    bad = np.zeros((m, n), bool)
    for j, p in enumerate(mi):
        big = rng.integers(p, 2**64 - 1, n, dtype=np.uint64, endpoint=True)
        sel = (np.arange(n) % m) == j
        x[j, sel] = big[sel]
        bad[j] = sel
    x[3, 5] = mi[3]                     # exactly p_j
    bad[3, 5] = True
    x[0, 7] = x[1, 7] = 2**64 - 1       # two limbs of one coefficient
    bad[0, 7] = bad[1, 7] = True
    d, w, f = exact(emu, mi, mo, x)
    plain = np.zeros((k, n), np.uint64)
    mi_, mo_ = _u(mi), _u(mo)
    assert emu.emu_bc_exact_plain(_p(mi_), m, _p(mo_), k, _p(x), n, _p(plain)) == 0
    assert (w == plain).all()
    wd, ww = py_exact(mi, mo, x)
    assert (d == wd).all() and (w == ww).all()
    assert (f[:m][bad] == OPERAND).all() and not f[:m][~bad].any() and not f[m:].any()
    # the fast form takes any word: the unchecked sums, no flag
    if fast_ok(m, mo):
        w, f = fast(emu, mi, mo, x)
        assert emu.emu_bc_fast_plain(_p(mi_), m, _p(mo_), k, _p(x), n, _p(plain)) == 0
        assert (w == plain).all() and (w == py_fast(mi, mo, x)).all()
        assert not f.any()
