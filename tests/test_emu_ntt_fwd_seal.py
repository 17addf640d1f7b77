"""CPU emulation of the sealed forward transform and of the sealed inverse with an output seal (tests/emu/emu_ntt_fwd_seal.cpp
compiles ntt_seal_tap.hpp with the very pass templates k_ntt_pass_sealed_io instantiates): the digest the loading launch forms is
the seal of the source whatever the tile order, the digest the storing launch forms is the seal of the row as stored, every
single-word change the seal promises to catch is caught on the load, the hooked tap changes words and digests together, and the
poison rule gives a raised row a seal that no verifier accepts -- without a GPU.

Every size 2^5 .. 2^20, both arithmetic paths, both directions.  Tiles per row (tiles()): one below 2^13; from there on the row
pass has N // 4096 and the column pass (1 << (logn - PC)) // 16 -- 16-column tiles of the 2^(logn - PC) columns, PC the stages of
the column plan of ntt_plan.hpp: PC = 5, 6, 7 at 2^13, 2^14, 2^15 and 8 from 2^16 on.  The forward transform loads with its column
pass and stores with its row pass, the inverse the other way round.  From 2^15 on a case samples its words and bits."""
import ctypes as C

import numpy as np
import pytest

from helpers.emu_build import build_emu
from helpers.sealed_case import py_seals
from helpers.sealed_ntt_runs import pow2_words
from oracle import cport as O

p64 = C.POINTER(C.c_uint64)
P = (1 << 61) - 1
SEAL_SUM, SEAL_RANGE = 1, 2
POISON = (1 << 64) - 1
SIZES = list(range(5, 21))
PATHS = [(0, 50), (1, 61)]
SAMPLED = 15      # from this size on: fewer words and bits per case
MAX_TILES = 256
PC = {13: 5, 14: 6, 15: 7, 16: 8, 17: 8, 18: 8, 19: 8, 20: 8}


def tiles(logn, inv):
    """(tiles of the loading launch, tiles of the storing launch) per row: the plan's formula"""
    if logn < 13:
        return 1, 1
    col, row = (1 << (logn - PC[logn])) // 16, (1 << logn) // 4096
    return (row, col) if inv else (col, row)


GRID = [(logn, path, bits, inv) for logn in SIZES for path, bits in PATHS for inv in (False, True)]
FWD = [g[:3] for g in GRID if not g[3]]


@pytest.fixture(scope="module")
def emu():
    L = build_emu("libemu_ntt_fwd_seal.so", ["emu_ntt_fwd_seal.cpp"], ("modarith.hpp", "ntt_core.hpp", "ntt_plan.hpp", "abft_taps.hpp", "seal_check.hpp",
                                                                       "ntt_seal_tap.hpp", "../../tests/emu/emu_ntt_seal.cpp"))
    L.emu_ntt_sealed_io.restype = C.c_int
    L.emu_ntt_sealed_io.argtypes = [C.c_int, p64, p64, C.c_int, C.c_uint64, p64, p64, C.c_int, C.c_longlong, C.c_int, p64, p64, p64, C.POINTER(C.c_int)]
    L.emu_ntt_seal_finish.restype = C.c_uint
    L.emu_ntt_seal_finish.argtypes = [p64, C.c_int, C.POINTER(C.c_int), p64, p64]
    L.emu_ntt_seal_out_finish.restype = None
    L.emu_ntt_seal_out_finish.argtypes = [p64, C.c_int, C.POINTER(C.c_int), C.c_uint, C.c_uint, p64]
    L.emu_seal_differs.restype = C.c_int
    L.emu_seal_differs.argtypes = [C.c_uint64, C.c_uint64, p64]
    return L


class Case:
    """One (size, path): modulus, tables, a clean row in [16, q - 16) and its seal, computed once."""

    def __init__(self, logn, path, bits):
        self.logn, self.path, self.N = logn, path, 1 << logn
        self.q = int(O.gen_primes(self.N, bits, 1)[0])
        self.rp = np.ascontiguousarray(O.root_powers(self.q, logn), dtype=np.uint64)
        rng = np.random.default_rng(300 * logn + path)
        self.w_hat = rng.integers(1, self.q, self.N, dtype=np.uint64)
        self.x = rng.integers(16, self.q - 16, self.N, dtype=np.uint64)
        self.seal = tuple(py_seals(self.x)[0])


_cases = {}


def case(logn, path, bits):
    if (logn, path) not in _cases:
        _cases[(logn, path)] = Case(logn, path, bits)
    return _cases[(logn, path)]


def oracle(c, src, inv):
    """the transform of the row as the unchecked transform takes it: a word >= q reduced first"""
    y = np.asarray(src, dtype=np.uint64) % np.uint64(c.q)
    return O.nwt_inverse(y, c.q, c.rp) if inv else O.nwt_forward(y, c.q, c.rp)


def run(emu, c, src, inv=False, hit=(-1, 0)):
    """(dst, parts_in [tin][3], parts_out [tout][2], (sum_in, sum_out)) of the sealed transform out of place from src"""
    src = np.ascontiguousarray(src, dtype=np.uint64)
    dst = np.zeros(c.N, dtype=np.uint64)
    pin, pout = np.zeros(3 * MAX_TILES, dtype=np.uint64), np.zeros(2 * MAX_TILES, dtype=np.uint64)
    sums = np.zeros(2, dtype=np.uint64)
    tiles = (C.c_int * 2)()
    rc = emu.emu_ntt_sealed_io(int(inv), src.ctypes.data_as(p64), dst.ctypes.data_as(p64), c.logn, c.q, c.rp.ctypes.data_as(p64), c.w_hat.ctypes.data_as(p64),
                               c.path, hit[0], hit[1], pin.ctypes.data_as(p64), pout.ctypes.data_as(p64), sums.ctypes.data_as(p64), tiles)
    assert rc == 0
    tin, tout = tiles[0], tiles[1]
    return dst, pin[:3 * tin].reshape(tin, 3), pout[:2 * tout].reshape(tout, 2), (int(sums[0]), int(sums[1]))


def finish_in(emu, parts, stored, order=None):
    """(flag, (S0, S1)) of k_ntt_seal_finish over the tiles in `order`"""
    tiles = len(parts)
    o = (C.c_int * tiles)(*(range(tiles) if order is None else order))
    got = np.zeros(2, dtype=np.uint64)
    st = np.array(stored, dtype=np.uint64) if stored is not None else None
    f = emu.emu_ntt_seal_finish(np.ascontiguousarray(parts).ctypes.data_as(p64), tiles, o, st.ctypes.data_as(p64) if st is not None else None, got.ctypes.data_as(p64))
    return int(f), (int(got[0]), int(got[1]))


def finish_out(emu, parts, flag_in=0, flag_abft=0, order=None):
    """the pair k_ntt_seal_out_finish writes for a row with those flags"""
    tiles = len(parts)
    o = (C.c_int * tiles)(*(range(tiles) if order is None else order))
    seal = np.zeros(2, dtype=np.uint64)
    emu.emu_ntt_seal_out_finish(np.ascontiguousarray(parts).ctypes.data_as(p64), tiles, o, flag_in, flag_abft, seal.ctypes.data_as(p64))
    return int(seal[0]), int(seal[1])


@pytest.mark.parametrize("logn,path,bits,inv", GRID)
def test_clean_row_both_digests_are_the_seals_in_any_tile_order(emu, logn, path, bits, inv):
    c = case(logn, path, bits)
    dst, pin, pout, sums = run(emu, c, c.x, inv)
    assert (len(pin), len(pout)) == tiles(logn, inv)
    want = oracle(c, c.x, inv)
    assert (dst == want).all()
    seal_dst = tuple(py_seals(want)[0])
    rng = np.random.default_rng(logn + 7 * path)
    for k in range(3):
        oi = [range(len(pin)), reversed(range(len(pin))), rng.permutation(len(pin))][k]
        oo = [range(len(pout)), reversed(range(len(pout))), rng.permutation(len(pout))][k]
        f, got = finish_in(emu, pin, c.seal, list(oi))
        assert got == c.seal and f == 0
        assert finish_out(emu, pout, order=list(oo)) == seal_dst
    assert finish_in(emu, pin, None)[0] == 0            # a null seal is not compared
    if not inv:                                        # the ABFT input side is the checked forward's: generate_weights on the words loaded
        p2 = 1 << (logn // 2)
        assert sums[0] == sum(((i % p2 + 1) + (i // p2 + 1)) * int(v) for i, v in enumerate(c.x)) % c.q


@pytest.mark.parametrize("logn,path,bits", FWD)
def test_single_bit_changes_move_the_sums_and_bit_63_raises_the_window(emu, logn, path, bits):
    c = case(logn, path, bits)
    for i, j in enumerate((0, c.N // 2 + 1, c.N - 1)):
        for bit in ((0, 40, 63) if logn < SAMPLED else (0, 40, 63)[i:i + 1]):
            y = c.x.copy()
            y[j] ^= np.uint64(1 << bit)
            dst, pin, pout, _ = run(emu, c, y)
            f, got = finish_in(emu, pin, c.seal)
            assert f & SEAL_SUM and got != c.seal and got == tuple(py_seals(y)[0]), (j, bit, f)
            assert bool(f & SEAL_RANGE) == (int(y[j]) >= c.q), (j, bit)
            if bit == 63:
                assert f & SEAL_RANGE
            # the words are the transform of the row as it is, and the output digest is the seal of those words
            want = oracle(c, y, False)
            assert (dst == want).all() and finish_out(emu, pout) == tuple(py_seals(want)[0])
            assert finish_out(emu, pout, flag_in=f) == (POISON, POISON)


@pytest.mark.parametrize("logn,path,bits", FWD)
def test_a_change_the_32_bit_fold_cannot_see_is_seen(emu, logn, path, bits):
    c = case(logn, path, bits)
    j, b = c.N // 3, 7
    v = (int(c.x[j]) | (1 << (b + 32))) & ~(1 << b)      # a word with bit b clear and bit b + 32 set
    base = c.x.copy()
    base[j] = np.uint64(v)
    y = base.copy()
    y[j] = np.uint64(v + (1 << b) - (1 << (b + 32)))
    assert (int(y[j]) - v) % ((1 << 32) - 1) == 0 and int(y[j]) < c.q
    stored = tuple(py_seals(base)[0])
    assert finish_in(emu, run(emu, c, base)[1], stored)[0] == 0
    assert finish_in(emu, run(emu, c, y)[1], stored)[0] == SEAL_SUM


@pytest.mark.parametrize("logn,path,bits,inv", GRID)
def test_hooked_tap_changes_words_and_digests_together(emu, logn, path, bits, inv):
    c = case(logn, path, bits)
    clean = run(emu, c, c.x, inv)[0]
    # word 0, a word inside another column tile and row tile, the last word
    for j, bit in ((0, 3), (min(c.N // 2 + 21, c.N - 2), 40), (c.N - 1, 63)):
        src = c.x.copy()
        dst, pin, pout, _ = run(emu, c, src, inv, hit=(j, bit))
        assert (src == c.x).all()                      # the source array is untouched
        y = c.x.copy()
        y[j] ^= np.uint64(1 << bit)
        want, wpin, wpout, _ = run(emu, c, y, inv)     # the same change made in memory
        assert (dst == want).all() and (pin == wpin).all() and (pout == wpout).all()
        assert not (dst == clean).all()
        f, got = finish_in(emu, pin, c.seal)
        assert got == tuple(py_seals(y)[0]) and f & SEAL_SUM
        assert bool(f & SEAL_RANGE) == (int(y[j]) >= c.q)


@pytest.mark.parametrize("logn,path,bits", [f for f in FWD if f[0] in (5, 14, 20)])      # the smallest size, two launches, the largest
def test_poison_rule(emu, logn, path, bits):
    c = case(logn, path, bits)
    _, _, pout, _ = run(emu, c, c.x)
    canonical = tuple(py_seals(oracle(c, c.x, False))[0])
    assert finish_out(emu, pout, 0, 0) == canonical
    for fi, fa in ((SEAL_SUM, 0), (SEAL_RANGE, 0), (SEAL_SUM | SEAL_RANGE, 0), (0, 1), (SEAL_SUM, 1), (0, 0x80000000)):
        assert finish_out(emu, pout, fi, fa) == (POISON, POISON), (fi, fa)
    # a poisoned pair differs from every digest, the row's own and the all-ones words included
    poison = np.array([POISON, POISON], dtype=np.uint64)
    ok = np.array(canonical, dtype=np.uint64)
    rng = np.random.default_rng(logn)
    digests = [canonical, (0, 0), (P - 1, P - 1), (P, P), (POISON, POISON)] + [tuple(int(v) for v in rng.integers(0, 1 << 63, 2, dtype=np.uint64)) for _ in range(8)]
    for s0, s1 in digests:
        assert emu.emu_seal_differs(s0, s1, poison.ctypes.data_as(p64)) == 1
    assert emu.emu_seal_differs(canonical[0], canonical[1], ok.ctypes.data_as(p64)) == 0
    assert emu.emu_seal_differs(canonical[0] + P, canonical[1], ok.ctypes.data_as(p64)) == 0      # a lazily reduced digest of the same residue


@pytest.mark.parametrize("logn,path,bits,inv", [g for g in GRID if g[0] < 18])
def test_hook_on_both_sides_of_every_power_of_two_moves_the_digest_by_that_words_weight(emu, logn, path, bits, inv):
    """The words 2^k - 1 and 2^k for every k and N - 1 hold both sides of the first edge of any tile size, column tiles included.
    Bit 3 flipped in word j on the load moves S0 by d = +-8 and S1 by (j + 1) d: the weight names the word, so the input digest
    proves that the hook hit word j of its tile and no other, and the output digest is the seal of the transform of that row.
    Below 2^18, where a case stays within a few seconds; test_gpu_sealed_sizes.py holds every size on the device."""
    c = case(logn, path, bits)
    for j in pow2_words(logn):
        dst, pin, pout, _ = run(emu, c, c.x, inv, hit=(j, 3))
        d = -8 if int(c.x[j]) & 8 else 8
        f, got = finish_in(emu, pin, c.seal)
        assert got == ((c.seal[0] + d) % P, (c.seal[1] + (j + 1) * d) % P) and f == SEAL_SUM, j
        if logn < SAMPLED:
            y = c.x.copy()
            y[j] ^= np.uint64(8)
            want = oracle(c, y, inv)
            assert (dst == want).all() and finish_out(emu, pout) == tuple(py_seals(want)[0]), j
