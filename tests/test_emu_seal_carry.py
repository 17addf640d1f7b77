"""CPU emulation of the carried add / subtract (tests/emu/emu_seal_carry.cpp compiles seal_carry.hpp, the per-word step and the
per-row prediction the kernels of seal_carry.hip call): the seal and locator predicted from the operands' sums and the counted wraps
equal Python-integer sums over the words actually produced, whatever the chunking, and each of the five fault points gives the
outcome the header promises -- without a GPU.

Every expected value is a Python integer computed here.  No trial is filtered out: where a flipped operand bit leaves the window
[0, q) the row must raise the range bit as well, and the test says which case it is in from the operands alone."""
import ctypes as C

import numpy as np
import pytest

from helpers.emu_build import build_emu
from oracle import cport as O

p64 = C.POINTER(C.c_uint64)
P = (1 << 61) - 1
SUM, RANGE = 1, 2
BITS = [30, 50, 61]
# (n, log_chunk): a row shorter than a workgroup; 2^13 as one chunk and cut smaller
CUTS = [(1 << 5, 5), (1 << 13, 13), (1 << 13, 10), (1 << 13, 6)]
PRIMES = {(bits, n): O.gen_primes(n, bits, 1)[0] for bits in BITS for n in (1 << 5, 1 << 13)}


@pytest.fixture(scope="module")
def emu():
    L = build_emu("libemu_seal_carry.so", ["emu_seal_carry.cpp"], ("modarith.hpp", "residue_check.hpp", "seal_check.hpp", "seal_carry.hpp"))
    L.emu_carry.restype = C.c_uint32
    L.emu_carry.argtypes = [p64, p64, p64, C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.c_int, p64, p64, p64, C.c_int, C.c_uint32, C.c_int]
    L.emu_carry_predict.restype = C.c_uint64
    L.emu_carry_predict.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int]
    L.emu_carry_fold32_equal.restype = C.c_int
    L.emu_carry_fold32_equal.argtypes = [C.c_uint64, C.c_uint64]
    return L


def _p(a):
    return a.ctypes.data_as(p64)


def sums(x):
    """{S0, S1, S2} of a row, Python integers"""
    row = [int(v) for v in x]
    return [sum(row) % P, sum((j + 1) * v for j, v in enumerate(row)) % P, sum((j + 1) ** 2 * v for j, v in enumerate(row)) % P]


def op(a, b, q, sub):
    """fhe_modadd's / fhe_modsub's words for any 64-bit operands, Python integers"""
    return [((int(x) % q) - (int(y) % q)) % q if sub else ((int(x) % q) + (int(y) % q)) % q for x, y in zip(a, b)]


def carry(emu, a, b, q, sub, loc, log_chunk, sa=None, sb=None, fault=(-1, 0, 0)):
    """(words, predicted sums [2 or 3], flags) of one row; sa / sb default to the true sums of a / b"""
    a, b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
    sa = np.array(sums(a) if sa is None else sa, dtype=np.uint64)
    sb = np.array(sums(b) if sb is None else sb, dtype=np.uint64)
    c = np.full(a.size, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    pred = np.full(3, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    fl = emu.emu_carry(_p(a), _p(b), _p(c), a.size, q, int(sub), int(loc), log_chunk, _p(sa), _p(sb), _p(pred), *fault)
    return c, [int(v) for v in pred[:3 if loc else 2]], fl


def designed(rng, q, n, sub):
    """(name, a, b): the rows the wrap count has to get right"""
    full = lambda v: np.full(n, v, dtype=np.uint64)
    rnd = lambda lo=0: rng.integers(lo, q, n, dtype=np.uint64)
    a, a1 = rnd(), rnd(1)
    rows = [("random", rnd(), rnd()), ("random2", rnd(), rnd()),
            ("all q - 1", full(q - 1), full(q - 1)),                            # add: every word wraps, E0 = N
            ("all zero", full(0), full(0)),
            ("sum q - 1", a, (q - 1 - a.astype(object)).astype(np.uint64)),     # add: the largest sum that does not wrap
            ("sum q", a1, (q - a1.astype(object)).astype(np.uint64))]           # add: exactly q, wraps to 0
    if sub:
        rows += [("a = b", a, a.copy()), ("0 - (q - 1)", full(0), full(q - 1))]
    return rows


@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("bits", BITS)
def test_predicted_seal_and_locator_equal_python_sums_of_the_actual_words(emu, bits, sub):
    for n in (1 << 5, 1 << 13):
        q = PRIMES[bits, n]
        for name, a, b in designed(np.random.default_rng(bits + n + sub), q, n, sub):
            assert (a < np.uint64(q)).all() and (b < np.uint64(q)).all()
            want_c = op(a, b, q, sub)
            want_s = sums(want_c)
            if not sub and name == "all q - 1":
                assert want_c == [q - 2] * n
            if not sub and name == "sum q":
                assert want_c == [0] * n
            if not sub and name == "sum q - 1":
                assert want_c == [q - 1] * n
            for loc in (False, True):
                for nn, log_chunk in CUTS:
                    if nn != n:
                        continue
                    c, pred, fl = carry(emu, a, b, q, sub, loc, log_chunk)
                    assert c.tolist() == want_c, (name, loc, log_chunk)
                    assert pred == want_s[:len(pred)] and len(pred) == (3 if loc else 2), (name, loc, log_chunk)
                    assert fl == 0, (name, loc, log_chunk)


def test_prediction_is_the_linear_identity(emu):
    q = PRIMES[61, 1 << 13]
    for sa, sb, E in ((0, 0, 0), (P - 1, P - 1, 1 << 13), (5, P - 3, (1 << 60) + 12345), (P - 1, 0, P - 1)):
        assert emu.emu_carry_predict(sa, sb, q, E, 0) == (sa + sb - q * E) % P
        assert emu.emu_carry_predict(sa, sb, q, E, 1) == (sa - sb + q * E) % P


def _operands(rng, q, n):
    """random operands whose words stay in the window whichever way bit 3 flips"""
    a, b = rng.integers(16, q - 16, n, dtype=np.uint64), rng.integers(16, q - 16, n, dtype=np.uint64)
    return a, b


@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("loc", [False, True])
@pytest.mark.parametrize("bits", BITS)
def test_each_fault_point_gives_its_outcome(emu, bits, loc, sub):
    for n, log_chunk in ((1 << 5, 5), (1 << 13, 13), (1 << 13, 9)):
        q = PRIMES[bits, n]
        a, b = _operands(np.random.default_rng(7 * bits + n), q, n)
        true_c = op(a, b, q, sub)
        true_s = sums(true_c)[:3 if loc else 2]
        for coeff in (0, n // 2, n - 1):
            for bit in (3, bits - 2):
                where = (bits, n, log_chunk, coeff, bit)
                # 0, 1: an operand word after its load -- the digest is of the words produced from it, the prediction is not
                for point, x in ((0, a), (1, b)):
                    c, pred, fl = carry(emu, a, b, q, sub, loc, log_chunk, fault=(point, coeff, bit))
                    hit = int(x[coeff]) ^ (1 << bit)
                    assert fl == (SUM if hit < q else SUM | RANGE), (point,) + where
                    y = (a if point else x).copy(), (x if point else b).copy()
                    y[point][coeff] = hit
                    assert c.tolist() == op(y[0], y[1], q, sub), (point,) + where
                    assert pred != sums(c)[:len(pred)], (point,) + where
                # 2: c before the digest and the store -- raised, and the stored word is wrong
                c, pred, fl = carry(emu, a, b, q, sub, loc, log_chunk, fault=(2, coeff, bit))
                assert fl == SUM, where
                assert [j for j in range(n) if int(c[j]) != true_c[j]] == [coeff] and int(c[coeff]) == true_c[coeff] ^ (1 << bit), where
                # 3: c after the digest -- nothing now; the seal written is that of the right words, so the next verification raises
                c, pred, fl = carry(emu, a, b, q, sub, loc, log_chunk, fault=(3, coeff, bit))
                assert fl == 0 and pred == true_s, where
                assert [j for j in range(n) if int(c[j]) != true_c[j]] == [coeff] and int(c[coeff]) == true_c[coeff] ^ (1 << bit), where
                got = sums(c)[:len(pred)]
                assert all(g != w for g, w in zip(got, pred)), where
                # 4: the wrap bit as counted -- the words are right
                c, pred, fl = carry(emu, a, b, q, sub, loc, log_chunk, fault=(4, coeff, bit))
                assert fl == SUM and c.tolist() == true_c, where
    # the hook is a function of the armed word alone: none armed, nothing raised
    assert carry(emu, a, b, q, sub, loc, log_chunk)[2] == 0


@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("bits", BITS)
def test_changes_a_fold_modulo_2_32_minus_1_cannot_see_are_caught(emu, bits, sub):
    n, log_chunk = 1 << 13, 13
    q = PRIMES[bits, n]
    rng = np.random.default_rng(bits)
    a, b = _operands(rng, q, n)
    # +2^b - 2^(b + 32) inside one word of a, between sealing and the add
    for j, bit in ((0, 3), (n // 2, 17), (n - 1, 27)):
        lo, hi = 5 + (1 << bit), 5 + (1 << (bit + 32))
        # where the window is too narrow to hold 2^(b + 32) the change runs the other way and the new word leaves the window
        sealed_word, now_word = (hi, lo) if hi < q else (lo, hi)
        sealed = a.copy()
        sealed[j] = sealed_word
        now = sealed.copy()
        now[j] = now_word
        assert emu.emu_carry_fold32_equal(sealed_word, now_word) and sealed_word < q
        c, pred, fl = carry(emu, now, b, q, sub, True, log_chunk, sa=sums(sealed))
        assert fl == (SUM if now_word < q else SUM | RANGE), (j, bit)
        assert c.tolist() == op(now, b, q, sub)
        # the same change in b
        assert carry(emu, b, now, q, sub, False, log_chunk, sb=sums(sealed))[2] == (SUM if now_word < q else SUM | RANGE), (j, bit)
    # d1 = -d2 on two words whose distance is a multiple of 3 * 5 * 17: S0 does not move, S1 does
    a, b = _operands(rng, q, n)
    sa = sums(a)
    for j1, j2 in ((0, 255), (1000, 1000 + 255 * 20), (n - 1 - 255 * 32, n - 1)):
        for d in (1, 1 << 20, 12345):
            now = a.copy()
            d = min(d, int(a[j2]), q - 1 - int(a[j1]))
            assert d > 0
            now[j1] += np.uint64(d)
            now[j2] -= np.uint64(d)
            assert sums(now)[0] == sa[0] and (now < np.uint64(q)).all()
            for loc in (False, True):
                assert carry(emu, now, b, q, sub, loc, log_chunk, sa=sa)[2] == SUM, (j1, j2, d, loc)
            # the same change in b
            assert carry(emu, b, now, q, sub, False, log_chunk, sb=sa)[2] == SUM, (j1, j2, d)


@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("bits", BITS)
def test_an_operand_word_outside_the_window_raises_range_and_keeps_the_unchecked_words(emu, bits, sub):
    n, log_chunk = 1 << 13, 10
    q = PRIMES[bits, n]
    a, b = _operands(np.random.default_rng(3 * bits), q, n)
    sa, sb = sums(a), sums(b)
    # words that were never canonical, sealed as they are: the range bit; the reduced word is not the sealed one, so the sum bit too
    for j, v in ((0, q), (n // 2, 2 * q + 5), (n - 1, (1 << 64) - 1)):
        for which in (0, 1):
            x = [a.copy(), b.copy()]
            x[which][j] = v
            c, pred, fl = carry(emu, x[0], x[1], q, sub, False, log_chunk, sa=sums(x[0]), sb=sums(x[1]))
            assert c.tolist() == op(x[0], x[1], q, sub), (j, v, which)
            assert fl & RANGE, (j, v, which)
    # a single-bit flip of a sealed word that leaves the window raises both bits: q never divides 2^b
    for j in (0, n // 2 + 1, n - 1):
        for bit in range(bits, 64, 7):
            for which in (0, 1):
                x = [a.copy(), b.copy()]
                x[which][j] ^= np.uint64(1 << bit)
                assert int(x[which][j]) >= q
                c, pred, fl = carry(emu, x[0], x[1], q, sub, True, log_chunk, sa=sa, sb=sb)
                assert fl == SUM | RANGE, (j, bit, which)
                assert c.tolist() == op(x[0], x[1], q, sub)


def test_a_raised_row_stays_raised_through_later_carried_adds(emu):
    n, log_chunk = 1 << 13, 13
    q = PRIMES[50, n]
    rng = np.random.default_rng(99)
    a, b = _operands(rng, q, n)
    sa = sums(a)
    a[77] ^= np.uint64(8)                                        # at rest, after sealing
    c, pred, fl = carry(emu, a, b, q, False, True, log_chunk, sa=sa)
    assert fl == SUM and pred != sums(c)
    for step in range(3):
        d = rng.integers(0, q, n, dtype=np.uint64)
        c, pred, fl = carry(emu, c, d, q, step == 1, True, log_chunk, sa=pred)
        assert fl == SUM, step
    # a stored sum that is not canonical is held word for word, as fhe_seal_verify holds it
    a, b = _operands(rng, q, n)
    sa = sums(a)
    if sa[0] + P < 1 << 64:
        assert carry(emu, a, b, q, False, False, log_chunk, sa=[sa[0] + P, sa[1], sa[2]])[2] == SUM
