"""CPU emulation of the sealed inverse transform's first launch (tests/emu/emu_ntt_seal.cpp compiles ntt_seal_tap.hpp with the very
pass templates k_ntt_pass_sealed_io instantiates): the digest the pass forms from the words it loads is the seal of seal_check.hpp
whatever the tile order, every single-word change the seal promises to catch is caught on that load, and the hooked tap changes
the words and the digest together while the source stays clean -- without a GPU.

Every size 2^5 .. 2^20, both arithmetic paths.  The first launch has one tile below 2^13 and N // 4096 from there on: the inverse
row pass holds 4096 points per tile at every two-launch size (PlanGeom::TR of ntt_plan.hpp: 16, 16, 16, 16, 8, 4, 2, 1 rows of
2^PR = 2^8 .. 2^12 points, PR = logn - PC with PC = 5, 6, 7, 8, 8, 8, 8, 8 for 2^13 .. 2^20).  From 2^15 on a case samples its words
and bits (SAMPLED) so that it stays within a few seconds on the host."""
import ctypes as C

import numpy as np
import pytest

from helpers.emu_build import build_emu
from helpers.sealed_ntt_runs import pow2_words
from oracle import cport as O

p64 = C.POINTER(C.c_uint64)
P = (1 << 61) - 1
SEAL_SUM, SEAL_RANGE = 1, 2
SIZES = list(range(5, 21))
SAMPLED = 15      # from this size on: a sample of the tile edges, one bit per word
MAX_TILES = 256
PATHS = [(0, 50), (1, 61)]


@pytest.fixture(scope="module")
def emu():
    L = build_emu("libemu_ntt_seal.so", ["emu_ntt_seal.cpp"], ("modarith.hpp", "ntt_core.hpp", "ntt_plan.hpp", "abft_taps.hpp", "seal_check.hpp",
                                                               "ntt_seal_tap.hpp"))
    L.emu_ntt_seal_first.restype = C.c_int
    L.emu_ntt_seal_first.argtypes = [p64, p64, C.c_int, C.c_uint64, p64, p64, C.c_int, C.c_int, C.c_longlong, C.c_int, p64, p64]
    L.emu_ntt_seal_finish.restype = C.c_uint
    L.emu_ntt_seal_finish.argtypes = [p64, C.c_int, C.POINTER(C.c_int), p64, p64]
    return L


class Case:
    """One (size, path): modulus, tables, a clean row in [16, q - 16) and its seal, computed once."""

    def __init__(self, logn, path, bits):
        self.logn, self.path, self.N = logn, path, 1 << logn
        self.q = int(O.gen_primes(self.N, bits, 1)[0])
        self.rp = np.ascontiguousarray(O.root_powers(self.q, logn), dtype=np.uint64)
        rng = np.random.default_rng(100 * logn + path)
        self.w_hat = rng.integers(1, self.q, self.N, dtype=np.uint64)
        self.x = rng.integers(16, self.q - 16, self.N, dtype=np.uint64)
        self.seal = seal_of(self.x)


_cases = {}


def case(logn, path, bits):
    if (logn, path) not in _cases:
        _cases[(logn, path)] = Case(logn, path, bits)
    return _cases[(logn, path)]


def seal_of(x):
    """S0 = sum x_j, S1 = sum (j + 1) x_j modulo 2^61 - 1 in Python integers."""
    return sum(int(v) for v in x) % P, sum((j + 1) * int(v) for j, v in enumerate(x)) % P


def first(emu, c, src, mode=1, hit=(-1, 0)):
    """(dst, parts [tiles][3], sum_in) of the first launch out of place from src."""
    src = np.ascontiguousarray(src, dtype=np.uint64)
    dst = np.zeros(c.N, dtype=np.uint64)
    parts = np.zeros(3 * MAX_TILES, dtype=np.uint64)
    s = np.zeros(1, dtype=np.uint64)
    tiles = emu.emu_ntt_seal_first(src.ctypes.data_as(p64), dst.ctypes.data_as(p64), c.logn, c.q, c.rp.ctypes.data_as(p64), c.w_hat.ctypes.data_as(p64), c.path,
                                   mode, hit[0], hit[1], parts.ctypes.data_as(p64), s.ctypes.data_as(p64))
    assert tiles > 0
    return dst, parts[:3 * tiles].reshape(tiles, 3), int(s[0])


def finish(emu, parts, stored, order=None):
    """(flag, (S0, S1)) of the finish step over the tiles in `order`."""
    tiles = len(parts)
    order = list(range(tiles)) if order is None else list(order)
    o = (C.c_int * tiles)(*order)
    got = np.zeros(2, dtype=np.uint64)
    st = np.array(stored, dtype=np.uint64) if stored is not None else None
    f = emu.emu_ntt_seal_finish(np.ascontiguousarray(parts).ctypes.data_as(p64), tiles, o, st.ctypes.data_as(p64) if st is not None else None,
                                got.ctypes.data_as(p64))
    return int(f), (int(got[0]), int(got[1]))


def verdict(emu, c, src):
    _, parts, _ = first(emu, c, src)
    return finish(emu, parts, c.seal)[0]


def edges(c, parts):
    """first word, last word and both sides of every tile edge; from 2^SAMPLED on of the first, the middle and the last edge"""
    tiles = len(parts)
    tile = c.N // tiles
    idx = {0, c.N - 1}
    for t in (range(1, tiles) if c.logn < SAMPLED else (1, tiles // 2, tiles - 1)):
        idx |= {t * tile - 1, t * tile}
    return sorted(idx)


@pytest.mark.parametrize("logn", SIZES)
@pytest.mark.parametrize("path,bits", PATHS)
def test_clean_row_digest_is_the_seal_in_any_tile_order(emu, logn, path, bits):
    c = case(logn, path, bits)
    dst, parts, s_in = first(emu, c, c.x)
    tiles = len(parts)
    assert tiles == (c.N // 4096 if logn >= 13 else 1)
    rng = np.random.default_rng(logn)
    for order in (range(tiles), reversed(range(tiles)), rng.permutation(tiles)):
        f, got = finish(emu, parts, c.seal, order)
        assert got == c.seal and f == 0
    assert finish(emu, parts, None)[0] == 0            # a null seal is not compared
    # the words are the untapped pass's, and the ABFT sum is the checked inverse's own
    plain, _, _ = first(emu, c, c.x, mode=0)
    assert (dst == plain).all()
    ref, _, s_ref = first(emu, c, c.x, mode=2)
    assert (ref == plain).all() and s_in == s_ref
    assert s_in == sum(int(a) * int(b) for a, b in zip(c.w_hat, c.x)) % c.q
    if logn < 13:                                      # single pass: the final words
        assert (dst == O.nwt_inverse(c.x, c.q, c.rp)).all()


@pytest.mark.parametrize("logn", SIZES)
@pytest.mark.parametrize("path,bits", PATHS)
def test_single_bit_changes_raise_the_sum_and_bit_63_the_window(emu, logn, path, bits):
    c = case(logn, path, bits)
    _, parts, _ = first(emu, c, c.x)
    bits = (0, 31, 32, 52, 60)
    for i, j in enumerate(edges(c, parts)):
        for bit in (bits if logn < SAMPLED else bits[i % 5:i % 5 + 1]):
            y = c.x.copy()
            y[j] ^= np.uint64(1 << bit)
            f = verdict(emu, c, y)
            assert f & SEAL_SUM, (j, bit, f)
        if logn < SAMPLED or i % 2 == 0:
            y = c.x.copy()
            y[j] ^= np.uint64(1 << 63)
            assert verdict(emu, c, y) & SEAL_RANGE, j


@pytest.mark.parametrize("logn", SIZES)
@pytest.mark.parametrize("path,bits", PATHS)
def test_changes_the_32_bit_fold_cannot_see(emu, logn, path, bits):
    c = case(logn, path, bits)
    j = c.N // 3
    b = 7
    # +2^b - 2^(b+32) inside one word: zero modulo 2^32 - 1
    y = c.x.copy()
    v = int(y[j]) | (1 << (b + 32))
    v &= ~(1 << b)
    base = c.x.copy()
    base[j] = np.uint64(v)                             # a word with bit b clear and bit b + 32 set
    c2 = Case.__new__(Case)
    c2.__dict__.update(c.__dict__)
    c2.x, c2.seal = base, seal_of(base)
    y = base.copy()
    y[j] = np.uint64(v + (1 << b) - (1 << (b + 32)))
    assert (int(y[j]) - v) % ((1 << 32) - 1) == 0
    assert verdict(emu, c2, base) == 0
    assert verdict(emu, c2, y) & SEAL_SUM
    # two words swapped: S0 stays, S1 moves
    y = c.x.copy()
    k = c.N - 2
    assert y[j] != y[k]
    y[j], y[k] = y[k], y[j]
    _, parts, _ = first(emu, c, y)
    f, got = finish(emu, parts, c.seal)
    assert got[0] == c.seal[0] and got[1] != c.seal[1] and f == SEAL_SUM


@pytest.mark.parametrize("logn", SIZES)
@pytest.mark.parametrize("path,bits", PATHS)
def test_non_canonical_stored_seal_counts_as_different(emu, logn, path, bits):
    c = case(logn, path, bits)
    _, parts, _ = first(emu, c, c.x)
    assert finish(emu, parts, (c.seal[0] + P, c.seal[1]))[0] == SEAL_SUM
    assert finish(emu, parts, (c.seal[0], c.seal[1] + P))[0] == SEAL_SUM


@pytest.mark.parametrize("logn", SIZES)
@pytest.mark.parametrize("path,bits", PATHS)
def test_hooked_tap_changes_words_and_digest_together(emu, logn, path, bits):
    c = case(logn, path, bits)
    clean, parts0, _ = first(emu, c, c.x)
    for j, bit in ((0, 3), (c.N // 2, 40), (c.N - 1, 63)):
        src = c.x.copy()
        dst, parts, _ = first(emu, c, src, hit=(j, bit))
        assert (src == c.x).all()                      # the source array is untouched
        y = c.x.copy()
        y[j] ^= np.uint64(1 << bit)
        want, wparts, _ = first(emu, c, y)             # the same change made in memory
        assert (dst == want).all() and (parts == wparts).all()
        assert not (dst == clean).all()
        f, got = finish(emu, parts, c.seal)
        assert got != c.seal or bit == 63
        assert f & (SEAL_RANGE if bit == 63 else SEAL_SUM)


def swept_words(logn):
    """pow2_words, every k below 2^18; every second k at 2^18 and every fourth from 2^19 on, so that a case stays within a few
    seconds on the host -- test_gpu_sealed_sizes.py holds every k at those sizes on the device"""
    step = 1 if logn < 18 else 2 if logn == 18 else 4
    keep = {w for k in range(0, logn, step) for w in ((1 << k) - 1, 1 << k)} | {(1 << logn) - 1}
    return [w for w in pow2_words(logn) if w in keep]


@pytest.mark.parametrize("logn", SIZES)
@pytest.mark.parametrize("path,bits", PATHS)
def test_hook_on_both_sides_of_every_power_of_two_moves_the_digest_by_that_words_weight(emu, logn, path, bits):
    """Every tile edge of every plan lies at a multiple of a power of two, so the words 2^k - 1 and 2^k hold both sides of the first
    edge of any tile size.  Bit 3 flipped in word j on the load moves S0 by d = +-8 and S1 by (j + 1) d: the weight names the word,
    so the digest proves that the hook hit word j of its tile and no other; below 2^SAMPLED the words are also held against the
    same change made in memory."""
    c = case(logn, path, bits)
    for j in swept_words(logn):
        dst, parts, _ = first(emu, c, c.x, hit=(j, 3))
        d = -8 if int(c.x[j]) & 8 else 8
        f, got = finish(emu, parts, c.seal)
        assert got == ((c.seal[0] + d) % P, (c.seal[1] + (j + 1) * d) % P) and f == SEAL_SUM, j
        if logn < SAMPLED:
            y = c.x.copy()
            y[j] ^= np.uint64(8)
            want, wparts, _ = first(emu, c, y)
            assert (dst == want).all() and (parts == wparts).all(), j
