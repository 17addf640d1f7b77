"""CPU emulation of the sealed Galois permutation (tests/emu/emu_galois_seal.cpp compiles galois_seal.hpp, the per-word step and
per-row verdict the kernels of galois_sealed.hip call, and walks a row the way the kernel cuts it): the gather-order digests are the
seals of source and destination whatever the chunking, every one-word and two-word change of the source raises the row -- the
patterns the 2^32 - 1 fold is blind to included --, an index fault raises a row of distinct words, and the written seal is {stored
S0, digested S1}, so a register fault poisons the destination's seal -- without a GPU."""
import ctypes as C

import numpy as np
import pytest

from helpers.emu_build import build_emu

p64 = C.POINTER(C.c_uint64)
P = (1 << 61) - 1
SUM, RANGE = 1, 2
WORD, INDEX = 0, 1
Q50 = 1125899904679937       # a 50-bit prime, 1 mod 2^15
Q61 = 2305843009211662337    # a 61-bit prime, 1 mod 2^15, below p
PATTERN = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def emu():
    L = build_emu("libemu_galois_seal.so", ["emu_galois_seal.cpp"], ("modarith.hpp", "ntt_core.hpp", "residue_check.hpp", "galois_check.hpp",
                                                                     "seal_check.hpp", "galois_seal.hpp"))
    L.emu_gs_slot.restype = C.c_uint32
    L.emu_gs_slot.argtypes = [C.c_uint32, C.c_int, C.c_uint32]
    L.emu_gs_permute.restype = C.c_uint32
    L.emu_gs_permute.argtypes = [p64, p64, C.c_int, C.c_uint32, C.c_uint64, C.c_int, p64, C.c_int, p64, p64, C.c_int, C.c_uint32, C.c_int]
    L.emu_gs_seal.restype = C.c_uint32
    L.emu_gs_seal.argtypes = [p64, C.c_uint32, C.c_uint64, p64, p64]
    L.emu_gs_fold32_equal.restype = C.c_int
    L.emu_gs_fold32_equal.argtypes = [C.c_uint64, C.c_uint64]
    return L


def _p(a):
    return a.ctypes.data_as(p64)


def py_seal(x):
    """(S0, S1) of a row in Python integers"""
    s0 = s1 = 0
    for j, v in enumerate(x.tolist()):
        s0 += v
        s1 += (j + 1) * v
    return s0 % P, s1 % P


def c_seal(emu, x, q, stored=None):
    x = np.ascontiguousarray(x, dtype=np.uint64)
    seal = np.zeros(2, dtype=np.uint64)
    f = emu.emu_gs_seal(_p(x), len(x), q, _p(seal), _p(stored) if stored is not None else None)
    return seal, f


def permute(emu, src, logn, k, q, stored, out=True, log_chunk=None, point=-1, coeff=0, bit=0):
    """-> (dst, seal_dst (pattern-filled when out is false), sums[4], flags)"""
    src = np.ascontiguousarray(src, dtype=np.uint64)
    dst = np.zeros_like(src)
    seal_dst = np.full(2, PATTERN, dtype=np.uint64)
    sums = np.zeros(4, dtype=np.uint64)
    lc = min(logn, 13) if log_chunk is None else log_chunk
    f = emu.emu_gs_permute(_p(src), _p(dst), logn, k, q, lc, _p(np.ascontiguousarray(stored, dtype=np.uint64)), 1 if out else 0, _p(seal_dst), _p(sums),
                           point, coeff, bit)
    return dst, seal_dst, sums, f


def elements(logn, rng):
    """every odd k for log N <= 4; above: k = 1, 2N - 1, the rotations' 5^i and a seeded sample"""
    two_n = 2 << logn
    if logn <= 4:
        return list(range(1, two_n, 2))
    ks = {1, two_n - 1} | {pow(5, i, two_n) for i in (1, 2, 3, 7)} | {int(2 * rng.integers(0, 1 << logn) + 1) for _ in range(4)}
    return sorted(ks)


LOGNS = (1, 4, 8, 10, 14)


def test_gather_order_digests_are_the_seals_of_source_and_destination(emu):
    rng = np.random.default_rng(19)
    for logn in LOGNS:
        N = 1 << logn
        for q in (Q50, Q61):
            src = rng.integers(0, q, N, dtype=np.uint64)
            want_src = py_seal(src) if logn <= 10 else tuple(int(v) for v in c_seal(emu, src, q)[0])
            if logn <= 10:
                assert tuple(int(v) for v in c_seal(emu, src, q)[0]) == want_src      # the C sweep used at 2^14 is the Python sum
            stored = np.array(want_src, dtype=np.uint64)
            ks = elements(logn, rng)
            for k in ks if logn < 14 else ks[:6]:
                slots = np.array([emu.emu_gs_slot(j, logn, k) for j in range(N)]) if logn <= 10 else None
                for lc in ((min(logn, 13),) if logn < 14 else (14, 13, 12)):
                    dst, seal_dst, sums, f = permute(emu, src, logn, k, q, stored, log_chunk=lc)
                    assert f == 0, (logn, k, lc)
                    if slots is not None:
                        assert np.array_equal(dst, src[slots])
                        assert sorted(slots.tolist()) == list(range(N))
                    want_dst, fd = c_seal(emu, dst, q)
                    assert fd == 0
                    if logn <= 10:
                        assert tuple(int(v) for v in want_dst) == py_seal(dst)
                    assert (int(sums[0]), int(sums[1])) == want_src, (logn, k, lc)
                    assert (int(sums[0]), int(sums[2])) == tuple(int(v) for v in want_dst), (logn, k, lc)
                    assert seal_dst.tolist() == want_dst.tolist()
                    assert int(sums[3]) == 0
                    # without a destination seal: same verdict, nothing written
                    dst2, seal2, sums2, f2 = permute(emu, src, logn, k, q, stored, out=False, log_chunk=lc)
                    assert f2 == 0 and np.array_equal(dst2, dst) and seal2.tolist() == [PATTERN] * 2 and sums2[:2].tolist() == sums[:2].tolist()


def one_word_changes(x, q, rng):
    """new values for a word x < q: single bits, x + p through the window, the pattern +2^b - 2^(b+32) the 2^32 - 1 fold cannot see"""
    out = [x ^ (1 << b) for b in (0, 31, 32, 49, 60, 63)]
    if x + P < (1 << 64):
        out.append(x + P)
    for b in (0, 7, 20):
        y = x + (1 << b) - (1 << (b + 32))
        if 0 <= y < (1 << 64):
            out.append(y)
        y = x - (1 << b) + (1 << (b + 32))
        if 0 <= y < (1 << 64):
            out.append(y)
    out.append(int(rng.integers(0, q)))
    return [v for v in out if v != x]


def test_every_one_word_change_of_the_source_raises_the_row(emu):
    rng = np.random.default_rng(23)
    blind = 0
    for logn in LOGNS:
        N = 1 << logn
        q = Q50 if logn % 2 == 0 else Q61
        src = rng.integers(0, q, N, dtype=np.uint64)
        stored, _ = c_seal(emu, src, q)
        k = elements(logn, rng)[1 if logn > 1 else 0]
        words = range(N) if logn <= 8 else sorted({0, 1, N - 1, N // 2 - 1, N // 2, (1 << min(logn, 13)) - 1, (1 << min(logn, 13)) % N} | set(rng.integers(0, N, 24).tolist()))
        for i in words:
            x = int(src[i])
            for y in one_word_changes(x, q, rng):
                bad = src.copy()
                bad[i] = y
                dst, seal_dst, sums, f = permute(emu, bad, logn, k, q, stored)
                assert f != 0, (logn, i, hex(x), hex(y))
                assert bool(f & RANGE) == (y >= q)
                if y < q:
                    assert f & SUM
                blind += emu.emu_gs_fold32_equal(x, y)
                # the destination carries the changed word and its seal fails: S0 is the stored one, or the window sees it
                assert int(np.count_nonzero(dst == np.uint64(y))) >= 1
                assert c_seal(emu, dst, q, seal_dst)[1] != 0
    assert blind > 0      # some of these changes are invisible modulo 2^32 - 1


def test_two_word_changes_raise_the_row(emu):
    rng = np.random.default_rng(29)
    for logn in (4, 8, 10, 14):
        N = 1 << logn
        q = Q61
        src = rng.integers(1 << 40, q - (1 << 40), N, dtype=np.uint64)
        stored, _ = c_seal(emu, src, q)
        k = pow(5, 3, 2 * N)
        for _ in range(40 if logn < 14 else 10):
            i, j = (int(v) for v in rng.choice(N, 2, replace=False))
            d = int(rng.integers(1, 1 << 39))
            bad = src.copy()
            # the sum-preserving pair +d / -d: S0 stays, S1 moves by (i - j) d != 0 mod p
            bad[i] = int(bad[i]) + d
            bad[j] = int(bad[j]) - d
            assert permute(emu, bad, logn, k, q, stored)[3] == SUM, (logn, i, j, d)
            bad[j] = int(rng.integers(0, q))
            assert permute(emu, bad, logn, k, q, stored)[3] & SUM


def test_an_index_fault_on_distinct_words_raises_the_row(emu):
    rng = np.random.default_rng(31)
    for logn in (1, 4, 8, 10, 14):
        N = 1 << logn
        q = Q50
        src = (rng.permutation(N).astype(np.uint64) * np.uint64(977) + np.uint64(5)) % np.uint64(q)      # pairwise distinct
        assert len(set(src.tolist())) == N
        stored, _ = c_seal(emu, src, q)
        for k in elements(logn, rng)[:4]:
            clean = permute(emu, src, logn, k, q, stored)[0]
            for coeff in sorted({0, N - 1, N // 2} | set(rng.integers(0, N, 3).tolist())):
                for bit in sorted({0, logn - 1}):
                    dst, seal_dst, sums, f = permute(emu, src, logn, k, q, stored, point=INDEX, coeff=coeff, bit=bit)
                    assert f == SUM, (logn, k, coeff, bit)
                    diff = np.flatnonzero(dst != clean)
                    assert diff.tolist() == [coeff]
                    assert dst[coeff] == src[emu.emu_gs_slot(coeff, logn, k) ^ (1 << bit)]
                    assert c_seal(emu, dst, q, seal_dst)[1] & SUM


def test_written_seal_is_stored_s0_and_digested_s1(emu):
    rng = np.random.default_rng(37)
    for logn in (4, 10, 14):
        N = 1 << logn
        q = Q61
        src = rng.integers(0, q, N, dtype=np.uint64)
        stored, _ = c_seal(emu, src, q)
        k = 2 * N - 1
        coeff, bit = int(rng.integers(0, N)), 17
        clean = permute(emu, src, logn, k, q, stored)[0]
        dst, seal_dst, sums, f = permute(emu, src, logn, k, q, stored, point=WORD, coeff=coeff, bit=bit)
        assert f & SUM
        assert np.flatnonzero(dst != clean).tolist() == [coeff] and int(dst[coeff]) == int(clean[coeff]) ^ (1 << bit)
        fresh, _ = c_seal(emu, dst, q)
        assert int(seal_dst[0]) == int(stored[0]) != int(fresh[0])      # carried, not re-digested
        assert int(seal_dst[1]) == int(fresh[1]) == int(sums[2])      # digested from the register that was stored
        assert c_seal(emu, dst, q, seal_dst)[1] & SUM      # the destination keeps failing
        # a stored S0 that is not canonical is held word for word: raised, and carried as it is
        odd = stored.copy()
        odd[0] = int(odd[0]) + P
        dst, seal_dst, sums, f = permute(emu, src, logn, k, q, odd)
        assert f == SUM and int(seal_dst[0]) == int(odd[0])
        # the hole: x + p keeps every sum; the window alone sees it, on this call and on the destination
        small = int(np.argmin(src))
        if int(src[small]) + P < (1 << 64):
            bad = src.copy()
            bad[small] = int(src[small]) + P
            dst, seal_dst, sums, f = permute(emu, bad, logn, k, q, stored)
            assert f == RANGE and int(sums[3]) == 1
            assert c_seal(emu, dst, q, seal_dst)[1] == RANGE
