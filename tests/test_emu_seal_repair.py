"""CPU emulation of the seal repair (tests/emu/emu_seal_repair.cpp compiles seal_check.hpp, the functions the kernels of
seal_repair.hip call): the arithmetic modulo p = 2^61 - 1 against Python integers, every single-word change located and restored
exactly, and every two-word change refused -- without a GPU.

The two-word traps are built on purpose: the same bit set in two words whose indices have an even sum, and d2 = -2^k d1 with an
integral weighted mean.  Each is first shown to be ACCEPTED by a locator made of S0 and S1 alone (it names an intact word), then to
be refused once S2 is held against it: that is what the third sum buys."""
import ctypes as C

import numpy as np
import pytest

from helpers.emu_build import build_emu
from oracle import cport as O

p64 = C.POINTER(C.c_uint64)
P = (1 << 61) - 1
CLEAN, REPAIRED, UNCORRECTABLE, TRANSIENT, SUSPECT = 0, 1, 2, 3, 4
BITS = [50, 61]
LOGNS = [1, 5, 13, 17]
PRIMES = {(bits, logn): O.gen_primes(1 << max(logn, 2), bits, 1)[0] for bits in BITS for logn in LOGNS}


@pytest.fixture(scope="module")
def emu():
    L = build_emu("libemu_seal_repair.so", ["emu_seal_repair.cpp"], ("modarith.hpp", "seal_check.hpp"))
    u64, u32 = C.c_uint64, C.c_uint32
    for name, res, args in (("emu_seal_mulmod", u64, [u64, u64]), ("emu_seal_inv", u64, [u64]), ("emu_seal_restore", u64, [u64, u64]),
                            ("emu_seal_locate", C.c_longlong, [u64, u64, u64, u32]), ("emu_seal3", None, [p64, C.c_size_t, u32, p64]),
                            ("emu_seal_locator", u64, [p64, u32]), ("emu_two_sum_locate", C.c_longlong, [u64, u64, u32]),
                            ("emu_seal_repair_row", None, [p64, u32, u64, p64, p64])):
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


def _p(a):
    return a.ctypes.data_as(p64)


def sums3(emu, x):
    x = np.ascontiguousarray(x, dtype=np.uint64)
    out = np.zeros(3, dtype=np.uint64)
    emu.emu_seal3(_p(x), 1, x.size, _p(out))
    return [int(v) for v in out]


def want3(x):
    v = [int(t) for t in x]
    return [sum(v) % P, sum((j + 1) * t for j, t in enumerate(v)) % P, sum((j + 1) ** 2 * t for j, t in enumerate(v)) % P]


def repair(emu, y, q, stored):
    """(report, the row afterwards) of k_row_repair's steps on a copy of y"""
    y = np.ascontiguousarray(y, dtype=np.uint64).copy()
    s = np.array(stored, dtype=np.uint64)
    rep = np.zeros(4, dtype=np.uint64)
    emu.emu_seal_repair_row(_p(y), y.size, q, _p(s), _p(rep))
    return [int(v) for v in rep], y


def syndromes(emu, y, stored):
    return [(g - s) % P for g, s in zip(sums3(emu, y), stored)]


@pytest.fixture(scope="module")
def rows(emu):
    """(x, q, its three sums) per (bits, logn), the sums held against Python integers once"""
    made = {}

    def get(bits, logn):
        if (bits, logn) not in made:
            n, q = 1 << logn, PRIMES[bits, logn]
            x = np.random.default_rng(100 * bits + logn).integers(0, q, n, dtype=np.uint64)
            s = sums3(emu, x)
            assert s == want3(x)
            made[bits, logn] = (x, q, s)
        return made[bits, logn]
    return get


def test_mulmod_and_inverse_against_python_integers(emu):
    rng = np.random.default_rng(7)
    edge = [0, 1, 2, P - 1, P - 2, 1 << 60, (1 << 32) - 1, 1 << 32]
    vals = edge + [int(v) for v in rng.integers(0, P, 200, dtype=np.uint64)]
    for a in edge:
        for b in vals:
            assert emu.emu_seal_mulmod(a, b) == a * b % P, (a, b)
    for a, b in zip(vals[8:108], vals[108:208]):
        assert emu.emu_seal_mulmod(a, b) == a * b % P, (a, b)
    assert emu.emu_seal_inv(0) == 0 and emu.emu_seal_inv(1) == 1 and emu.emu_seal_inv(P - 1) == P - 1
    for a in vals:
        if a:
            inv = emu.emu_seal_inv(a)
            assert inv == pow(a, P - 2, P) and inv * a % P == 1, a
    # restore: any 64-bit word, any canonical difference
    for x in (0, 1, P - 1, P, P + 1, 2**64 - 1, 2**63 + 12345):
        for d in (0, 1, P - 1, 2**60 + 3):
            assert emu.emu_seal_restore(x, d) == (x - d) % P, (x, d)


def test_the_locator_sum_at_2_17_where_the_square_of_the_weight_passes_2_32(emu, rows):
    x, q, s = rows(61, 17)
    assert (len(x)) ** 2 > 2**32
    assert s[2] == sum((j + 1) ** 2 * int(v) for j, v in enumerate(x)) % P
    assert emu.emu_seal_locator(_p(x), len(x)) == s[2]
    # any 64-bit words, the largest weights
    y = x.copy()
    y[-3:] = [2**64 - 1, P, 2**63]
    assert emu.emu_seal_locator(_p(y), len(y)) == want3(y)[2] == sums3(emu, y)[2]


@pytest.mark.parametrize("logn", LOGNS)
@pytest.mark.parametrize("bits", BITS)
def test_every_single_bit_of_a_word_is_located_and_restored(emu, rows, bits, logn):
    x, q, s = rows(bits, logn)
    n = len(x)
    assert repair(emu, x, q, s)[0] == [TRANSIENT, 0, 0, 0]      # a flagged row that is clean on the re-read
    for j in sorted({0, 1, n - 1}):
        for bit in range(64):
            y = x.copy()
            y[j] ^= np.uint64(1 << bit)
            d = syndromes(emu, y, s)
            assert emu.emu_seal_locate(*d, n) == j, (j, bit)
            assert emu.emu_seal_restore(int(y[j]), d[0]) == int(x[j]), (j, bit)
            rep, z = repair(emu, y, q, s)
            assert rep == [REPAIRED, j, int(y[j]), int(x[j])], (j, bit, rep)
            assert (z == x).all(), (j, bit)


@pytest.mark.parametrize("logn", LOGNS)
@pytest.mark.parametrize("bits", BITS)
def test_multi_bit_patterns_in_one_word(emu, rows, bits, logn):
    x, q, s = rows(bits, logn)
    n = len(x)
    rng = np.random.default_rng(bits + logn)
    for j in sorted({0, n // 2, n - 1}):
        patterns = []
        # x' = x + p: bits 0 and 61 flipped together on an odd word below 2^61 -- no sum moves, the window alone sees it
        x_odd = x.copy()
        x_odd[j] |= np.uint64(1)
        patterns.append((x_odd, int(x_odd[j]) ^ 1 ^ (1 << 61)))
        assert patterns[-1][1] == int(x_odd[j]) + P
        # x' >= 2^61: high bits set and low bits scrambled; three flipped bits; x' = x + 8 p, the largest multiple that fits
        patterns.append((x, int(x[j]) ^ int(rng.integers(1 << 61, 1 << 64, dtype=np.uint64))))
        patterns.append((x, int(x[j]) ^ 0b111 << 20))
        x_small = x.copy()
        x_small[j] = int(x[j]) % 8      # 2^64 - 8 p = 8
        patterns.append((x_small, int(x_small[j]) + 8 * P))
        if bits == 61:
            patterns.append((x, q + (P - q) // 2))      # inside [q, p)
            patterns.append((x, P - 1))
            patterns.append((x, q))
        for base, new in patterns:
            stored = s if base is x else sums3(emu, base)
            y = base.copy()
            y[j] = new
            rep, z = repair(emu, y, q, stored)
            assert rep == [REPAIRED, j, new, int(base[j])], (j, hex(new), rep)
            assert (z == base).all()
    y = x.copy()
    y[0] = int(x[0]) | 1
    stored = sums3(emu, y)
    y[0] = int(y[0]) + P
    assert syndromes(emu, y, stored) == [0, 0, 0]      # the x + p change: every syndrome is zero


def _trap_rows(x, q, n):
    """[(name, corrupted row, the intact word a two-sum locator names or None)] of two-word changes in the row x"""
    out = []
    bit = 7
    for j1, j2 in ((2, 10), (1, n - 1), (0, 2)):      # j1 + j2 even: the midpoint is a word of the row
        base = x.copy()
        base[[j1, j2]] &= ~np.uint64(1 << bit)
        y = base.copy()
        y[[j1, j2]] |= np.uint64(1 << bit)
        out.append((f"midpoint {j1} {j2}", base, y, (j1 + j2) // 2))
    # d1 = +2^b in word j1 (bit b 0 -> 1), d2 = -2^(b + k) in word j2 (bit b + k 1 -> 0): D1 / D0 = (2^k w2 - w1) / (2^k - 1)
    for k, j1, j2 in ((1, 4, 9), (2, 3, 9), (3, 5, 19)):
        w1, w2 = j1 + 1, j2 + 1
        assert ((w2 << k) - w1) % ((1 << k) - 1) == 0
        w = ((w2 << k) - w1) // ((1 << k) - 1)
        assert 1 <= w <= n and w not in (w1, w2)
        base = x.copy()
        base[j1] &= ~np.uint64(1 << bit)
        base[j2] |= np.uint64(1 << (bit + k))
        y = base.copy()
        y[j1] |= np.uint64(1 << bit)
        y[j2] &= ~np.uint64(1 << (bit + k))
        out.append((f"d2 = -2^{k} d1", base, y, w - 1))
    base = x.copy()
    base[5] = int(base[5]) // 2 + 1      # unequal words
    y = base.copy()
    y[[5, 20]] = base[[20, 5]]
    assert y[5] != base[5]
    out.append(("swapped", base, y, None))
    return out


@pytest.mark.parametrize("logn", [5, 13, 17])
@pytest.mark.parametrize("bits", BITS)
def test_two_word_changes_are_refused_where_two_sums_alone_would_miscorrect(emu, rows, bits, logn):
    x, q, _ = rows(bits, logn)
    n = len(x)
    for name, base, y, trap in _trap_rows(x, q, n):
        stored = sums3(emu, base)
        assert (y < np.uint64(q)).all() and int((y != base).sum()) == 2
        d = syndromes(emu, y, stored)
        if trap is not None:
            # what S2 buys: S0 and S1 alone name an intact word, in range, and "restoring" it gives a row that passes the seal
            assert emu.emu_two_sum_locate(d[0], d[1], n) == trap, name
            z = y.copy()
            z[trap] = emu.emu_seal_restore(int(y[trap]), d[0])
            assert y[trap] == base[trap] and z[trap] < q and sums3(emu, z)[:2] == stored[:2] and (z != base).sum() == 3, name
        else:
            assert d[0] == 0 and emu.emu_two_sum_locate(d[0], d[1], n) == -1
        assert emu.emu_seal_locate(*d, n) == -1, name
        rep, z = repair(emu, y, q, stored)
        assert rep == [UNCORRECTABLE, 0, 0, 0], (name, rep)
        assert (z == y).all(), name      # never written to


@pytest.mark.parametrize("bits", BITS)
def test_a_corrupted_stored_sum_never_causes_a_write(emu, rows, bits):
    x, q, s = rows(bits, 13)
    n = len(x)
    for which in range(3):
        for bit in (0, 17, 60, 61, 63):
            stored = list(s)
            stored[which] ^= 1 << bit
            rep, z = repair(emu, x, q, stored)
            assert rep == [SUSPECT, 0, 0, 0] and (z == x).all(), (which, bit)
        # a stored sum that is congruent but not canonical is a moved sum too
        stored = list(s)
        stored[which] += P
        assert repair(emu, x, q, stored)[0] == [SUSPECT, 0, 0, 0]
    # two stored sums moved, in any pair and such that D1 / D0 is in range: S2 disagrees
    for a, b in ((0, 1), (0, 2), (1, 2)):
        stored = list(s)
        stored[a], stored[b] = (stored[a] - 1) % P, (stored[b] - 5) % P
        rep, z = repair(emu, x, q, stored)
        assert rep == [UNCORRECTABLE, 0, 0, 0] and (z == x).all(), (a, b)
    assert emu.emu_two_sum_locate(1, 5, n) == 4
    # a corrupted stored sum beside a corrupted row: inconsistent, the row stays as it was found
    y = x.copy()
    y[n // 3] ^= np.uint64(1 << 9)
    for which in range(3):
        stored = list(s)
        stored[which] ^= 1 << 33
        rep, z = repair(emu, y, q, stored)
        assert rep == [UNCORRECTABLE, 0, 0, 0] and (z == y).all(), which
    # one sum moved and a word out of the window: not a suspect seal
    y = x.copy()
    y[3] = int(x[3]) | 1
    stored = sums3(emu, y)
    y[3] = int(y[3]) + P
    stored[1] ^= 4
    rep, z = repair(emu, y, q, stored)
    assert rep == [UNCORRECTABLE, 0, 0, 0] and (z == y).all()


@pytest.mark.parametrize("bits", BITS)
def test_window_disagreements_are_uncorrectable(emu, rows, bits):
    x, q, s = rows(bits, 5)
    # two words each moved by a multiple of p: no sum moves, two words out of the window
    y = x.copy()
    y[[3, 9]] = [int(x[3]) + P, int(x[9]) + 2 * P]
    rep, z = repair(emu, y, q, s)
    assert rep == [UNCORRECTABLE, 0, 0, 0] and (z == y).all()
    # a located word and ANOTHER word out of the window: x[4] changed inside the window, x[9] moved by p
    y = x.copy()
    y[4] ^= np.uint64(2)
    y[9] = int(x[9]) + P
    rep, z = repair(emu, y, q, s)
    assert rep == [UNCORRECTABLE, 0, 0, 0] and (z == y).all()
    # a consistent single-word syndrome whose restored word would not be below q: the stored sums are of a row with a word >= q
    if bits == 61:
        base = x.copy()
        base[6] = q + 1
        stored = sums3(emu, base)
        y = base.copy()
        y[6] = 12345
        rep, z = repair(emu, y, q, stored)
        assert rep == [UNCORRECTABLE, 0, 0, 0] and (z == y).all()
