"""CPU emulation of the checked rescale's residue stage (tests/emu/emu_rescale_check.cpp compiles rescale_check.hpp, the element
function the kernel of rescale_checked.hip calls): clean words equal Python's ``x % q_j`` with no flag, a bit flip at any
injection point raises a flag exactly when it changes the stored word, and x >= q_last raises bit 4 alone -- without a GPU.

Where the residue identity cannot see a change of the quotient, the windows must: as residue_check.hpp states for the products,
modulo m = 2^32 - 1 a change of k by a multiple of m / gcd(q, m) leaves k q unchanged (gcd > 1 only for 3, 5, 17, 257, 65537),
and so does a 64-bit wrap of the remainder by a multiple of m words (primes just below a power of two).  Neither case is
filtered out below: both are constructed on purpose and must come out flagged by the window bit alone."""
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
PRIMES = {bits: O.gen_primes(N, bits, 2) for bits in (30, 50, 61)}
# (q_last, q_j): every ordered pair of sizes, and two different primes of the same size in both orders
PAIRS = [(PRIMES[a][0], PRIMES[b][0]) for a in (30, 50, 61) for b in (30, 50, 61) if a != b] + \
        [(PRIMES[a][i], PRIMES[a][1 - i]) for a in (30, 50, 61) for i in (0, 1)]
IDS = [f"{ql.bit_length()}b{ql % 1000}-{qj.bit_length()}b{qj % 1000}" for ql, qj in PAIRS]


@pytest.fixture(scope="module")
def emu():
    L = build_emu("libemu_rescale_check.so", ["emu_rescale_check.cpp"], ("modarith.hpp", "residue_check.hpp", "rescale_check.hpp"))
    L.emu_rescale_reduce_checked.restype = C.c_int
    L.emu_rescale_reduce_checked.argtypes = [p64, C.c_size_t, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, p64, p32]
    L.emu_rescale_reduce_plain.restype = C.c_int
    L.emu_rescale_reduce_plain.argtypes = [p64, C.c_size_t, C.c_uint64, p64]
    return L


def _p(a):
    return a.ctypes.data_as(p64)


def reduce(emu, x, ql, qj, point=-1, mask=0):
    x = np.ascontiguousarray(x, dtype=np.uint64)
    w, f = np.zeros(x.size, dtype=np.uint64), np.zeros(x.size, dtype=np.uint32)
    assert emu.emu_rescale_reduce_checked(_p(x), x.size, ql, qj, point, mask, _p(w), f.ctypes.data_as(p32)) == 0
    return w, f


def _words(rng, ql, qj, n):
    """random words of [0, q_last) plus the edges 0, q_j - 1, q_j and q_last - 1 (those of them that are residues of q_last: the
    others belong to test_words_that_are_not_residues_of_the_dropped_prime)"""
    x = rng.integers(0, ql, n, dtype=np.uint64)
    edges = [e for e in (0, qj - 1, qj, ql - 1, 1, 2 * qj, 2 * qj - 1) if 0 <= e < ql]
    x[:len(edges)] = edges
    return x


@pytest.mark.parametrize("ql,qj", PAIRS, ids=IDS)
def test_clean_words_are_exact_and_raise_nothing(emu, ql, qj):
    x = _words(np.random.default_rng(ql % 9973 + qj % 7919), ql, qj, 5000)
    w, f = reduce(emu, x, ql, qj)
    assert [int(v) for v in w] == [int(v) % qj for v in x]
    assert not f.any()


@pytest.mark.parametrize("ql,qj", PAIRS, ids=IDS)
def test_flip_is_flagged_exactly_when_it_changes_the_word(emu, ql, qj):
    x = _words(np.random.default_rng(1 + ql % 9973 + qj % 7919), ql, qj, 300)
    clean, f0 = reduce(emu, x, ql, qj)
    assert not f0.any() and [int(v) for v in clean] == [int(v) % qj for v in x]
    for point in (PRODUCT, QUOTIENT, RESULT):
        flagged_and_changed = 0
        for bit in range(64):
            w, f = reduce(emu, x, ql, qj, point, 1 << bit)
            changed, flagged = w != clean, f != 0
            bad = np.nonzero(changed != flagged)[0]
            assert bad.size == 0, f"point {point} bit {bit}: x {x[bad[0]]} word {clean[bad[0]]} -> {w[bad[0]]}, flags {f[bad[0]]}"
            assert not (f & OPERAND).any()
            flagged_and_changed += int((flagged & changed).any())
            if point == RESULT:
                assert flagged.all() and changed.all(), f"bit {bit} of the result word not caught"
            elif bit >= 2:
                # the two conditional subtractions absorb an estimate up to two too low and nothing else
                assert flagged.all() and changed.all(), f"point {point} bit {bit}: a quotient off by 2^{bit} passed"
        assert flagged_and_changed >= 62
    # no running sum: the point does not exist
    w, f = np.zeros(x.size, dtype=np.uint64), np.zeros(x.size, dtype=np.uint32)
    assert emu.emu_rescale_reduce_checked(_p(x), x.size, ql, qj, SUM, 1, _p(w), f.ctypes.data_as(p32)) != 0


@pytest.mark.parametrize("ql,qj", PAIRS, ids=IDS)
def test_words_that_are_not_residues_of_the_dropped_prime(emu, ql, qj):
    """x >= q_last raises bit 4 alone, and the word is still the unchecked arithmetic's (x mod q_j for any 64-bit x)"""
    rng = np.random.default_rng(2 + ql % 9973 + qj % 7919)
    n = 400
    x = rng.integers(0, ql, n, dtype=np.uint64)
    big = rng.integers(ql, 2**64 - 1, n, dtype=np.uint64, endpoint=True)
    x[::3] = big[::3]
    x[1] = ql - 1
    x[3] = ql
    x[6] = 2**64 - 1
    for i, e in enumerate(e for e in (qj - 1, qj) if e >= ql):
        x[9 + 3 * i] = e
    bad = x >= np.uint64(ql)
    assert bad.any() and (~bad).any()
    w, f = reduce(emu, x, ql, qj)
    plain = np.zeros(n, dtype=np.uint64)
    assert emu.emu_rescale_reduce_plain(_p(x), n, qj, _p(plain)) == 0
    assert (w == plain).all()
    assert [int(v) for v in w] == [int(v) % qj for v in x]
    assert (f[bad] == OPERAND).all() and not f[~bad].any()


@pytest.mark.parametrize("qj", [3, 5, 17, 257, 65537])
def test_quotient_moved_by_a_multiple_of_m_over_q_is_left_to_the_window(emu, qj):
    """gcd(q_j, m) = q_j for the five prime factors of m = 2^32 - 1: a quotient that is off by m / q_j passes the residue identity
    (the remainder moves by exactly m).  The window has to catch it, and does."""
    ql = PRIMES[61][0]
    step = (2**32 - 1) // qj
    bits = step.bit_length()
    rng = np.random.default_rng(qj)
    # quotients whose low bits are zero, so that XOR with `step` ADDS it: x = (a << bits) q_j + delta
    a = rng.integers(1, (ql // qj) >> bits, 200, dtype=np.uint64)
    x = (a << np.uint64(bits)) * np.uint64(qj) + rng.integers(0, qj, 200, dtype=np.uint64)
    assert (x < np.uint64(ql)).all()
    clean, f0 = reduce(emu, x, ql, qj)
    assert not f0.any() and [int(v) for v in clean] == [int(v) % qj for v in x]
    w, f = reduce(emu, x, ql, qj, QUOTIENT, step)
    changed, flagged = w != clean, f != 0
    assert (changed == flagged).all()
    # wherever the word changed the quotient moved by about m / q_j and k q_j by about m: the identity cannot be relied on there
    # (it sees an exact move only through the 2^64 = 1 of a wrapped remainder), so the window bit itself must be raised
    assert changed.sum() >= 50 and ((f[changed] & RANGE) != 0).all() and not (f & OPERAND).any()


def test_remainder_wrapped_by_a_multiple_of_m_words_is_left_to_the_window(emu):
    """q = 2^50 - 2^18 + 1 (the arithmetic does not need it prime): 2^46 q = m 2^64 + 2^46, so a quotient estimate 2^46 too high
    leaves the remainder delta - 2^46 -- in [0, q) whenever delta >= 2^46 -- and the identity holds modulo m.  Only the quotient
    estimate's own window sees it."""
    ql, qj = PRIMES[61][0], 2**50 - 2**18 + 1
    rng = np.random.default_rng(46)
    x = rng.integers(0, ql, 400, dtype=np.uint64)
    clean, f0 = reduce(emu, x, ql, qj)
    assert not f0.any() and [int(v) for v in clean] == [int(v) % qj for v in x]
    for point in (PRODUCT, QUOTIENT):
        for bit in range(64):
            w, f = reduce(emu, x, ql, qj, point, 1 << bit)
            assert ((w != clean) == (f != 0)).all(), (point, bit)
        w, f = reduce(emu, x, ql, qj, point, 1 << 46)
        blind = clean >= np.uint64(2**46)
        assert blind.sum() >= 100
        assert (w[blind] == clean[blind] - np.uint64(2**46)).all() and (f[blind] == RANGE).all()
