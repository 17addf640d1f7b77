"""CPU emulation of the checked scalar multiply / affine map (tests/emu/emu_scalar_check.cpp compiles scalar_check.hpp, the element
function the kernel of scalar_checked.hip calls): clean words equal Python's ``(a * s + o) % q`` with no flag, a bit flip at any
injection point raises a flag exactly when it changes the stored word, and a >= q raises bit 4 alone -- without a GPU.

Where the residue identity cannot see a change of the quotient, the windows must.  Modulo m = 2^32 - 1 a change of k by m / q
leaves k q unchanged for the five prime factors of m, and a 64-bit wrap of the remainder by a multiple of m words is invisible too
(primes just below a power of two).  Neither case is filtered out below: both are constructed on purpose and must come out flagged
by the window bit."""
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
BITS = [30, 50, 61]


@pytest.fixture(scope="module")
def emu():
    L = build_emu("libemu_scalar_check.so", ["emu_scalar_check.cpp"], ("modarith.hpp", "residue_check.hpp", "scalar_check.hpp"))
    L.emu_scalar_affine_checked.restype = C.c_int
    L.emu_scalar_affine_checked.argtypes = [p64, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_uint64, p64, p32]
    L.emu_scalar_affine_plain.restype = C.c_int
    L.emu_scalar_affine_plain.argtypes = [p64, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint64, p64]
    return L


def _p(a):
    return a.ctypes.data_as(p64)


def affine(emu, a, q, s, o=None, point=-1, mask=0, status=0):
    """words and flags of a s (+ o) mod q; o None: no addend"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    w, f = np.zeros(a.size, dtype=np.uint64), np.zeros(a.size, dtype=np.uint32)
    rc = emu.emu_scalar_affine_checked(_p(a), a.size, q, s, 0 if o is None else o, int(o is not None), point, mask, _p(w), f.ctypes.data_as(p32))
    assert (rc == 0) == (status == 0)
    return w, f


def _words(rng, q, n):
    a = rng.integers(0, q, n, dtype=np.uint64)
    a[:3] = (0, 1, q - 1)
    return a


def _scalars(q):
    return [0, 1, q - 1, 65537 % q]


def _want(a, q, s, o):
    return [(int(v) * s + (o or 0)) % q for v in a]


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("add", [False, True])
def test_clean_words_are_exact_and_raise_nothing(emu, bits, add):
    q = PRIMES[bits]
    rng = np.random.default_rng(bits + 7 * add)
    a = _words(rng, q, 3000)
    for s in _scalars(q) + [int(rng.integers(0, q))]:
        for o in ([0, 1, q - 1, int(rng.integers(0, q))] if add else [None]):
            w, f = affine(emu, a, q, s, o)
            assert [int(v) for v in w] == _want(a, q, s, o), (s, o)
            assert not f.any(), (s, o)


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("add", [False, True])
def test_flip_is_flagged_exactly_when_it_changes_the_word(emu, bits, add):
    q = PRIMES[bits]
    rng = np.random.default_rng(100 + bits + 7 * add)
    a = _words(rng, q, 300)
    for s in (q - 1, 65537 % q, int(rng.integers(2, q))):
        o = int(rng.integers(0, q)) if add else None
        clean, f0 = affine(emu, a, q, s, o)
        assert not f0.any() and [int(v) for v in clean] == _want(a, q, s, o)
        for point in (PRODUCT, QUOTIENT, RESULT) + ((SUM,) if add else ()):
            caught = 0
            for bit in range(64):
                w, f = affine(emu, a, q, s, o, point, 1 << bit)
                changed, flagged = w != clean, f != 0
                bad = np.nonzero(changed != flagged)[0]
                assert bad.size == 0, f"s {s} point {point} bit {bit}: a {a[bad[0]]} word {clean[bad[0]]} -> {w[bad[0]]}, flags {f[bad[0]]}"
                assert not (f & OPERAND).any()
                caught += int((flagged & changed).any())
                if point != QUOTIENT:
                    # 2^b is never a multiple of q, nor 0 modulo m: a flip of the product, the sum or the word always shows
                    assert flagged.all() and changed.all(), f"point {point} bit {bit} not caught"
                elif bit >= 2:
                    # the two conditional subtractions absorb an estimate up to two too low and nothing else
                    assert flagged.all() and changed.all(), f"a quotient off by 2^{bit} passed"
            assert caught >= 62


@pytest.mark.parametrize("bits", BITS)
def test_the_sum_point_exists_only_with_an_addend(emu, bits):
    q = PRIMES[bits]
    a = _words(np.random.default_rng(bits), q, 16)
    affine(emu, a, q, 5, None, SUM, 1, status=-1)
    w, f = affine(emu, a, q, 5, 7, SUM, 1)
    assert (f != 0).all()
    affine(emu, a, q, 5, 7, 4, 1, status=-1)


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("add", [False, True])
def test_noncanonical_words_raise_bit_4_alone_and_keep_the_unchecked_word(emu, bits, add):
    q = PRIMES[bits]
    rng = np.random.default_rng(2 + bits + 7 * add)
    n = 400
    a = rng.integers(0, q, n, dtype=np.uint64)
    big = rng.integers(q, 2**64 - 1, n, dtype=np.uint64, endpoint=True)
    a[::3] = big[::3]
    a[1], a[3], a[6] = q - 1, q, 2**64 - 1
    bad = a >= np.uint64(q)
    assert bad.any() and (~bad).any()
    for s in (q - 1, 65537 % q, 1, 0):
        o = int(rng.integers(0, q)) if add else None
        w, f = affine(emu, a, q, s, o)
        plain = np.zeros(n, dtype=np.uint64)
        assert emu.emu_scalar_affine_plain(_p(a), n, q, s, o or 0, _p(plain)) == 0
        assert (w == plain).all()
        assert (f[bad] == OPERAND).all() and not f[~bad].any()
        # on canonical words the plain arithmetic is the exact one
        assert [int(v) for v in plain[~bad]] == _want(a[~bad], q, s, o)


@pytest.mark.parametrize("q", [3, 5, 17, 257, 65537])
def test_quotient_moved_by_m_over_q_is_left_to_the_window(emu, q):
    """gcd(q, m) = q for the five prime factors of m = 2^32 - 1: a quotient off by m / q moves k q by exactly m.  Products below q
    have quotient 0, so XOR with m / q ADDS it.  The window has to catch it, and does -- as it does every single-bit flip."""
    step = (2**32 - 1) // q
    pairs = [(x, s) for s in range(q if q < 300 else 40) for x in range(q if q < 300 else 1500) if x * s < q]
    for s in sorted({s for _, s in pairs}):
        a = np.array([x for x, s2 in pairs if s2 == s], dtype=np.uint64)
        clean, f0 = affine(emu, a, q, s)
        assert not f0.any() and [int(v) for v in clean] == _want(a, q, s, None)
        w, f = affine(emu, a, q, s, None, QUOTIENT, step)
        assert (w != clean).all() and ((f & RANGE) != 0).all() and not (f & OPERAND).any()
    rng = np.random.default_rng(q)
    a = rng.integers(0, q, 300, dtype=np.uint64)
    for s in (q - 1, int(rng.integers(1, q))):
        clean, _ = affine(emu, a, q, s, 1)
        assert [int(v) for v in clean] == _want(a, q, s, 1)
        for point in (PRODUCT, QUOTIENT, RESULT, SUM):
            for bit in range(64):
                w, f = affine(emu, a, q, s, 1, point, 1 << bit)
                assert ((w != clean) == (f != 0)).all(), (point, bit)


def test_remainder_wrapped_by_a_multiple_of_m_words_is_left_to_the_window(emu):
    """q = 2^50 - 2^18 + 1 (the arithmetic does not need it prime): 2^46 q = m 2^64 + 2^46, so a quotient estimate off by 2^46
    leaves the remainder c -+ 2^46 -- inside [0, q) for most c -- and the identity holds modulo m.  The quotient of a product is as
    large as a, so only its own window (the FP64 estimate) sees it."""
    q = 2**50 - 2**18 + 1
    rng = np.random.default_rng(46)
    a = rng.integers(0, q, 400, dtype=np.uint64)
    for s, o in ((q - 1, None), (int(rng.integers(q // 2, q)), None), (65537, None), (q - 2, 12345)):
        clean, f0 = affine(emu, a, q, s, o)
        assert not f0.any() and [int(v) for v in clean] == _want(a, q, s, o)
        for bit in range(64):
            w, f = affine(emu, a, q, s, o, QUOTIENT, 1 << bit)
            assert ((w != clean) == (f != 0)).all(), (s, bit)
        w, f = affine(emu, a, q, s, o, QUOTIENT, 1 << 46)
        moved = np.where(w > clean, w - clean, clean - w)
        blind = (w < np.uint64(q)) & (moved == np.uint64(2**46))
        assert blind.sum() >= 100, (s, int(blind.sum()))
        assert (f[blind] == RANGE).all()
