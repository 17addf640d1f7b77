"""CPU emulation of the sealed key-switch inner product (tests/emu/emu_ks_seal.cpp compiles ks_seal.hpp, the per-pair step and the
per-row decision the kernels of keyswitch_sealed.hip call): the words are the inner product's on both arithmetic paths and in every
instantiated band of digits, the 2 dnum digests of a row equal Python-integer sums whatever the chunking, the lanes and the order of
merging, and a fault on the load moves exactly the digest of the key row it hits and that half's output word while the residue
identity goes on holding -- without a GPU.

Every expected value is a Python integer computed here."""
import ctypes as C

import numpy as np
import pytest

from helpers.emu_build import build_emu
from helpers.stream_cases import barrett_shortfall, fp64_edge_pairs, small_residue_pairs
from oracle import cport as O

p64, p32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
P = (1 << 61) - 1
SUM, RANGE = 1, 2
PW_OPERAND = 4
F64, U64 = 0, 1
# (bits, path): the FP64-term form exists below 2^50 only
PATHS = [(50, F64), (50, U64), (61, U64)]
LOGNS = [1, 5, 13, 14]
PRIMES = {(bits, logn): O.gen_primes(1 << logn, bits, 1)[0] for bits in (50, 61) for logn in LOGNS}
BANDS = (2, 4, 8, 12)
CAP = BANDS[-1]
# every band, its upper edge and a dnum strictly inside it: 1 | 2 || 3 | 4 || 5 | 8 || 11 | 12
DNUMS = (1, 2, 3, 4, 5, 8, CAP - 1, CAP)


def band(dnum):
    return next(b for b in BANDS if dnum <= b)


@pytest.fixture(scope="module")
def emu():
    L = build_emu("libemu_ks_seal.so", ["emu_ks_seal.cpp"], ("modarith.hpp", "residue_check.hpp", "seal_check.hpp", "bsgs_check.hpp", "bsgs_seal.hpp",
                                                             "ks_seal.hpp"))
    L.emu_ks_seal_max_dnum.restype = C.c_uint
    L.emu_ks_sealed.restype = C.c_int
    L.emu_ks_sealed.argtypes = [p64, p64, p64, C.c_uint32, C.c_uint32, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, p64, C.c_int,
                                C.c_uint32, C.c_int, p64, p64, p32, p64, p32]
    return L


def sums(x):
    """[S0, S1] of a row, Python integers"""
    row = [int(v) for v in x]
    return [sum(row) % P, sum((j + 1) * v for j, v in enumerate(row)) % P]


def key_sums(key):
    """the seals of key rows 2 d + h of key [dnum][2][n]"""
    return [sums(key[d][h]) for d in range(key.shape[0]) for h in range(2)]


def product(c, ext, key, q, own):
    """both halves of the inner product for any 64-bit words, Python integers"""
    dnum, n = key.shape[0], key.shape[2]
    xs = [[int(v) for v in (c if d == own else ext[d])] for d in range(dnum)]
    return [[sum(xs[d][i] * int(key[d][h][i]) for d in range(dnum)) % q for i in range(n)] for h in range(2)]


def sealed(emu, c, ext, key, q, path, own=-1, nd=None, log_chunk=None, lanes=256, reverse=False, seal=None, hit=(-1, 0, -1)):
    """(words [2], residue flags [2], digests [2 dnum][2], key-row flags [2 dnum]); seal defaults to the true sums of the key rows"""
    c, ext, key = (np.ascontiguousarray(x, dtype=np.uint64) for x in (c, ext, key))
    dnum, n = key.shape[0], key.shape[2]
    assert ext.shape == (dnum, n) and c.shape == (n,) and key.shape == (dnum, 2, n)
    log_chunk = min(n.bit_length() - 1, 13) if log_chunk is None else log_chunk
    seal = np.array(key_sums(key) if seal is None else seal, dtype=np.uint64).reshape(4 * dnum)
    acc = [np.full(n, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64) for _ in range(2)]
    fl, sf = np.full(2, 0xA5A5A5A5, dtype=np.uint32), np.full(2 * dnum, 0xA5A5A5A5, dtype=np.uint32)
    dig = np.full(4 * dnum, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    u = lambda a: a.ctypes.data_as(p64)
    rc = emu.emu_ks_sealed(u(c), u(ext), u(key), n, dnum, own, q, path, band(dnum) if nd is None else nd, log_chunk, lanes, int(reverse), u(seal), hit[0], hit[1],
                           hit[2], u(acc[0]), u(acc[1]), fl.ctypes.data_as(p32), u(dig), sf.ctypes.data_as(p32))
    assert rc == 0
    return acc, fl.tolist(), [[int(v) for v in dig[2 * i:2 * i + 2]] for i in range(2 * dnum)], sf.tolist()


def random_case(rng, q, n, dnum, lo=0, hi=None):
    hi = q if hi is None else hi
    return rng.integers(lo, hi, n, dtype=np.uint64), rng.integers(lo, hi, (dnum, n), dtype=np.uint64), rng.integers(lo, hi, (dnum, 2, n), dtype=np.uint64)


def test_the_cap_is_the_largest_band(emu):
    assert emu.emu_ks_seal_max_dnum() == CAP
    assert [band(d) for d in DNUMS] == [2, 2, 4, 4, 8, 8, 12, 12]


@pytest.mark.parametrize("bits,path", PATHS)
@pytest.mark.parametrize("logn", LOGNS)
def test_words_and_digests_in_every_band(emu, bits, path, logn):
    n, q = 1 << logn, PRIMES[bits, logn]
    dnums = DNUMS if logn <= 5 else (3, CAP) if logn == 13 else (2, 5)
    for dnum in dnums:
        rng = np.random.default_rng(1000 * logn + 10 * dnum + bits + path)
        c, ext, key = random_case(rng, q, n, dnum)
        # the row inside a digit's own limb range (x from c: the first and the last digit) and outside every one (x from ext)
        for own in sorted({-1, 0, dnum - 1}):
            want = product(c, ext, key, q, own)
            acc, fl, dig, sf = sealed(emu, c, ext, key, q, path, own=own)
            assert [a.tolist() for a in acc] == want, (dnum, own)
            assert fl == [0, 0] and sf == [0] * (2 * dnum), (dnum, own)
            assert dig == key_sums(key), (dnum, own)
        if own != -1:
            assert want != product(c, ext, key, q, -1)      # the choice of x matters to the words
        # a band wider than it has to be gives the same words and digests
        if band(dnum) != CAP:
            assert sealed(emu, c, ext, key, q, path, nd=CAP)[2] == key_sums(key)


@pytest.mark.parametrize("bits,path", PATHS)
def test_designed_rows_pass(emu, bits, path):
    logn = 5
    n, q = 1 << logn, PRIMES[bits, logn]
    rng = np.random.default_rng(bits + path)
    full = lambda v, *shape: np.full(shape, v, dtype=np.uint64)
    for dnum in (1, 3, 8, CAP):
        rows = [("all q - 1", full(q - 1, n), full(q - 1, dnum, n), full(q - 1, dnum, 2, n)), ("all zero", full(0, n), full(0, dnum, n), full(0, dnum, 2, n))]
        # key words whose product with the digit lies next to a multiple of q: Barrett's estimate is one short there, and the FP64
        # form's sign fix decides the word
        pairs = small_residue_pairs(q, n, rng) if path == U64 else fp64_edge_pairs(q, n, rng)
        a, b = np.array([p[0] for p in pairs], dtype=np.uint64), np.array([p[1] for p in pairs], dtype=np.uint64)
        rows.append(("small residues", a, np.stack([a] * dnum), np.stack([np.stack([b, b])] * dnum)))
        for name, c, ext, key in rows:
            want = product(c, ext, key, q, 0)
            if name == "all q - 1":
                assert want[0] == [dnum % q] * n
            if name == "small residues" and path == U64 and dnum == 1:
                assert any(barrett_shortfall(int(x) * int(y), q) for x, y in zip(a, b)), "the designed pairs never needed Barrett's conditional subtraction"
            acc, fl, dig, sf = sealed(emu, c, ext, key, q, path, own=0)
            assert [x.tolist() for x in acc] == want, (name, dnum)
            assert fl == [0, 0] and sf == [0] * (2 * dnum) and dig == key_sums(key), (name, dnum)


def test_digests_do_not_depend_on_chunks_lanes_or_merge_order(emu):
    n, q, dnum = 1 << 14, PRIMES[61, 14], 3
    c, ext, key = random_case(np.random.default_rng(14), q, n, dnum)
    ref = sealed(emu, c, ext, key, q, U64, own=1)
    assert ref[2] == key_sums(key)
    for log_chunk, lanes, reverse in ((13, 256, True), (14, 256, False), (9, 256, True), (6, 64, False), (1, 1, True), (13, 1024, False), (4, 2, True)):
        got = sealed(emu, c, ext, key, q, U64, own=1, log_chunk=log_chunk, lanes=lanes, reverse=reverse)
        assert got[2] == ref[2] and got[3] == [0] * (2 * dnum) and got[1] == [0, 0], (log_chunk, lanes, reverse)
        assert all((x == y).all() for x, y in zip(got[0], ref[0]))
    # n = 2: one lane, two words
    n, q = 2, PRIMES[50, 1]
    c, ext, key = random_case(np.random.default_rng(1), q, n, CAP)
    assert sealed(emu, c, ext, key, q, F64, log_chunk=1, lanes=256)[2] == sealed(emu, c, ext, key, q, F64, log_chunk=1, lanes=1)[2] == key_sums(key)


@pytest.mark.parametrize("bits,path", PATHS)
def test_a_key_word_outside_the_window_raises_its_row_and_is_not_fixed(emu, bits, path):
    logn = 5
    n, q = 1 << logn, PRIMES[bits, logn]
    for dnum in (2, 5, CAP):
        c, ext, key = random_case(np.random.default_rng(dnum + bits + path), q, n, dnum)
        seal = key_sums(key)
        for d, h, j in ((0, 0, 0), (dnum - 1, 1, n - 1), (dnum // 2, 1, 7)):
            # x -> x + p: no sum moves, the window alone sees it
            now = key.copy()
            assert int(now[d][h][j]) + P < 1 << 64
            now[d][h][j] += np.uint64(P)
            acc, fl, dig, sf = sealed(emu, c, ext, now, q, path, own=0, seal=seal)
            assert sf == [RANGE if r == 2 * d + h else 0 for r in range(2 * dnum)], (dnum, d, h, j)
            assert dig == seal
            # the product is that of the word as it is; the residue check cannot cover it and says so on that half only
            assert [x.tolist() for x in acc] == product(c, ext, now, q, 0)
            assert fl == [PW_OPERAND if hh == h else 0 for hh in range(2)]
            # x -> q exactly: the window and the sums
            now = key.copy()
            now[d][h][j] = np.uint64(q)
            acc, fl, dig, sf = sealed(emu, c, ext, now, q, path, own=0, seal=seal)
            assert sf == [(SUM | RANGE) if r == 2 * d + h else 0 for r in range(2 * dnum)]
            assert [x.tolist() for x in acc] == product(c, ext, now, q, 0)


@pytest.mark.parametrize("bits,path", PATHS)
def test_a_fault_on_the_load_moves_its_rows_digest_and_its_halfs_word_only(emu, bits, path):
    for logn, log_chunk, dnums in ((5, 5, (1, 3, 8, CAP)), (14, 13, (3,))):
        n, q = 1 << logn, PRIMES[bits, logn]
        for dnum in dnums:
            c, ext, key = random_case(np.random.default_rng(7 * bits + logn + path + dnum), q, n, dnum, lo=16, hi=q - 16)      # bit 3 never leaves the window
            own = dnum - 1
            clean = sealed(emu, c, ext, key, q, path, own=own, log_chunk=log_chunk)
            assert clean[3] == [0] * (2 * dnum) and clean[1] == [0, 0]
            for d, h in sorted({(0, 0), (0, 1), (dnum - 1, 0), (dnum - 1, 1), (dnum // 2, 1)}):
                for coeff in (0, n // 2 - 1, n // 2, n - 1):
                    r = 2 * d + h
                    where = (dnum, d, h, coeff)
                    acc, fl, dig, sf = sealed(emu, c, ext, key, q, path, own=own, log_chunk=log_chunk, hit=(r, coeff, 3))
                    assert sf == [SUM if i == r else 0 for i in range(2 * dnum)], where
                    assert fl == [0, 0], where      # the identity holds on the key as loaded
                    faulted = key.copy()
                    faulted[d][h][coeff] ^= np.uint64(8)
                    assert dig[r] == sums(faulted[d][h]) and all(a != b for a, b in zip(dig[r], clean[2][r])), where
                    assert all(dig[i] == clean[2][i] for i in range(2 * dnum) if i != r), where
                    assert (acc[1 - h] == clean[0][1 - h]).all(), where
                    diff = np.flatnonzero(acc[h] != clean[0][h]).tolist()
                    assert diff == [coeff], where
                    x = int(c[coeff]) if d == own else int(ext[d][coeff])
                    assert int(acc[h][coeff]) == (int(clean[0][h][coeff]) + x * (int(faulted[d][h][coeff]) - int(key[d][h][coeff]))) % q, where


@pytest.mark.parametrize("bits,path", PATHS)
def test_at_rest_changes_and_wrong_seals_raise_their_row_only(emu, bits, path):
    logn, dnum = 14, 3
    n, q = 1 << logn, PRIMES[bits, logn]
    c, ext, key = random_case(np.random.default_rng(bits + path), q, n, dnum, lo=16, hi=q - 16)
    seal = key_sums(key)
    only = lambda r, v: [v if i == r else 0 for i in range(2 * dnum)]
    for d, h in ((0, 0), (1, 1), (2, 1)):
        r = 2 * d + h
        # one word, both sides of the chunk edge and the row's ends: the sum bit on that key row only; the identity holds
        for j in (0, (1 << 13) - 1, 1 << 13, n - 1):
            now = key.copy()
            now[d][h][j] ^= np.uint64(8)
            acc, fl, dig, sf = sealed(emu, c, ext, now, q, path, own=0, seal=seal)
            assert sf == only(r, SUM) and fl == [0, 0], (d, h, j)
        # two words by +d and -d: S0 does not move, S1 does
        now = key.copy()
        now[d][h][100] += np.uint64(5)
        now[d][h][100 + 255 * 20] -= np.uint64(5)
        assert sums(now[d][h])[0] == seal[r][0]
        assert sealed(emu, c, ext, now, q, path, own=0, seal=seal)[3] == only(r, SUM)
        # a changed seal word, and a stored sum that is not canonical
        for w in (0, 1):
            bad = [list(s) for s in seal]
            bad[r][w] ^= 1 << 17
            assert sealed(emu, c, ext, key, q, path, own=0, seal=bad)[3] == only(r, SUM), (d, h, w)
        for w in (0, 1):
            if seal[r][w] + P < 1 << 64:
                bad = [list(s) for s in seal]
                bad[r][w] += P
                assert sealed(emu, c, ext, key, q, path, own=0, seal=bad)[3] == only(r, SUM), (d, h, w)
