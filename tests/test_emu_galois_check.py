"""CPU emulation of the checked NTT-domain Galois permutation (tests/emu/emu_galois_check.cpp compiles galois_check.hpp, the
element functions the kernel of galois_checked.hip calls): the slot maps of k and k^-1 are inverse permutations, the slot map is
the automorphism of the oracle, clean sums agree, every single-bit flip of a moved word is flagged, and every single-bit flip of
a source index is flagged unless the weighted residues of the two words coincide -- without a GPU."""
import ctypes as C

import numpy as np
import pytest

from helpers.emu_build import build_emu
from oracle import cport as O
from oracle.keyswitch_ref import galois_coeff

p64 = C.POINTER(C.c_uint64)
p32 = C.POINTER(C.c_uint32)
WORD, INDEX = 0, 1
M32 = (1 << 32) - 1


@pytest.fixture(scope="module")
def emu():
    L = build_emu("libemu_galois_check.so", ["emu_galois_check.cpp"], ("modarith.hpp", "ntt_core.hpp", "residue_check.hpp", "galois_check.hpp"))
    L.emu_galois_slot.restype = C.c_uint32
    L.emu_galois_slot.argtypes = [C.c_uint32, C.c_int, C.c_uint32]
    L.emu_galois_permute.restype = C.c_int
    L.emu_galois_permute.argtypes = [p64, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint64, C.c_int, p64, p64, p64, p32]
    return L


def _slots(emu, logn, k):
    return np.array([emu.emu_galois_slot(j, logn, k) for j in range(1 << logn)], dtype=np.int64)


def permute(emu, src, logn, k, point=-1, unit=0, coeff=0, bit=0):
    """src: [units][N] -> (dst, s_in, s_out, flags)"""
    src = np.ascontiguousarray(src, dtype=np.uint64)
    units = src.shape[0]
    kinv = pow(k, -1, 2 << logn)
    dst = np.zeros_like(src)
    s_in, s_out, flags = np.zeros(units, dtype=np.uint64), np.zeros(units, dtype=np.uint64), np.zeros(units, dtype=np.uint32)
    assert emu.emu_galois_permute(src.ctypes.data_as(p64), units, logn, k, kinv, point, unit, coeff, bit, dst.ctypes.data_as(p64),
                                  s_in.ctypes.data_as(p64), s_out.ctypes.data_as(p64), flags.ctypes.data_as(p32)) == 0
    return dst, s_in, s_out, flags


def _res(x):
    return int(x) % M32


def test_slot_maps_of_k_and_its_inverse_are_inverse_permutations(emu):
    """(a) every odd k at log_n = 5, a seeded sample at log_n = 10 and 16"""
    rng = np.random.default_rng(1)
    for logn, ks in ((5, range(1, 64, 2)), (10, 2 * rng.integers(0, 1 << 10, 12) + 1), (16, 2 * rng.integers(0, 1 << 16, 4) + 1)):
        N = 1 << logn
        js = np.arange(N) if logn < 16 else rng.integers(0, N, 2048)
        for k in ks:
            k = int(k)
            kinv = pow(k, -1, 2 * N)
            for j in js:
                assert emu.emu_galois_slot(emu.emu_galois_slot(int(j), logn, k), logn, kinv) == j, (logn, k, j)


@pytest.mark.parametrize("logn", [5, 10])
def test_slot_map_is_the_automorphism_of_the_oracle(emu, logn):
    """(b) permuting the forward transform by pi_k = the forward transform of x -> x^k on the coefficients"""
    N = 1 << logn
    qs = O.gen_primes(N, 50, 1) + O.gen_primes(N, 61, 1)
    rps = np.stack([O.root_powers(q, logn) for q in qs])
    rng = np.random.default_rng(logn)
    x = np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs])
    X = O.nwt_forward_batch(x, qs, rps)
    for k in (3, 5, 25, 2 * N - 1, N + 1):
        want = O.nwt_forward_batch(np.stack([galois_coeff(x[l], k, q) for l, q in enumerate(qs)]), qs, rps)
        pi = _slots(emu, logn, k)
        assert (X[:, pi] == want).all(), k
        dst, _, _, flags = permute(emu, X, logn, k)
        assert (dst == want).all() and not flags.any(), k


@pytest.mark.parametrize("logn", [5, 8, 10, 13])
def test_clean_sums_agree_and_equal_python_integers(emu, logn):
    """(c)"""
    N = 1 << logn
    rng = np.random.default_rng(100 + logn)
    src = rng.integers(0, 1 << 64, (3, N), dtype=np.uint64)
    src[0, :4] = [0, M32, (1 << 64) - 1, 1 << 32]           # both spellings of the residue 0, and a carry between the halves
    for k in (1, 3, 5, 125, 2 * N - 1):
        dst, s_in, s_out, flags = permute(emu, src, logn, k)
        pi = _slots(emu, logn, k)
        assert (dst == src[:, pi]).all()
        assert not flags.any()
        for u in range(3):
            want = sum((j + 1) * _res(dst[u, j]) for j in range(N)) % M32
            assert _res(s_out[u]) == want and _res(s_in[u]) == want, (k, u)


def test_every_bit_flip_of_a_moved_word_is_flagged(emu):
    """(d) all 64 bits, on words that include 0, 2^32 - 1 and 2^64 - 1, first / middle / last position of a row"""
    logn, N = 5, 32
    rng = np.random.default_rng(7)
    src = rng.integers(0, 1 << 64, (3, N), dtype=np.uint64)
    src[1, :3] = [0, M32, (1 << 64) - 1]
    n = 0
    for k in (3, 2 * N - 1):
        clean = permute(emu, src, logn, k)[0]
        kinv = pow(k, -1, 2 * N)
        # destination positions: the ends, the middle, and where the three special words of unit 1 land
        coeffs = [0, 17, N - 1] + [emu.emu_galois_slot(i, logn, kinv) for i in range(3)]
        for unit, coeff in [(0, c) for c in coeffs[:3]] + [(1, c) for c in coeffs[3:]] + [(2, N - 1)]:
            for bit in range(64):
                dst, _, _, flags = permute(emu, src, logn, k, WORD, unit, coeff, bit)
                assert flags.tolist() == [int(u == unit) for u in range(3)], (k, unit, coeff, bit)
                diff = np.argwhere(dst != clean).tolist()
                assert diff == [[unit, coeff]] and int(dst[unit, coeff]) == int(clean[unit, coeff]) ^ (1 << bit)
                n += 1
    assert n == 2 * 7 * 64


@pytest.mark.parametrize("logn", [5, 10])
def test_every_bit_flip_of_a_source_index_is_flagged(emu, logn):
    """(e) flagged whenever w(j) (r(x') - r(x)) != 0 modulo 2^32 - 1, the condition evaluated here in Python integers; with
    these seeds no case falls under the exception"""
    N = 1 << logn
    rng = np.random.default_rng(900 + logn)
    src = rng.integers(0, 1 << 64, (2, N), dtype=np.uint64)
    n = 0
    for k in (5, 2 * N - 1):
        pi = _slots(emu, logn, k)
        coeffs = range(N) if logn == 5 else [0, 1, 341, N // 2, N - 2, N - 1]
        for coeff in coeffs:
            for bit in range(logn):
                unit = (coeff + bit) & 1
                x, x2 = int(src[unit, pi[coeff]]), int(src[unit, pi[coeff] ^ (1 << bit)])
                caught = ((coeff + 1) * (_res(x2) - _res(x))) % M32 != 0
                assert caught, "a committed seed must not fall under the exception"
                dst, _, _, flags = permute(emu, src, logn, k, INDEX, unit, coeff, bit)
                assert int(dst[unit, coeff]) == x2
                assert flags.tolist() == [int(u == unit) for u in range(2)], (k, coeff, bit)
                n += 1
    assert n == 2 * logn * (N if logn == 5 else 6)


def test_points_that_do_not_exist_are_refused(emu):
    src = np.zeros((1, 32), dtype=np.uint64)
    d = np.zeros_like(src)
    s, f = np.zeros(2, dtype=np.uint64), np.zeros(1, dtype=np.uint32)
    args = lambda point, unit, coeff, bit: emu.emu_galois_permute(src.ctypes.data_as(p64), 1, 5, 3, 43, point, unit, coeff, bit, d.ctypes.data_as(p64),
                                                                  s.ctypes.data_as(p64), s[1:].ctypes.data_as(p64), f.ctypes.data_as(p32))
    assert args(INDEX, 0, 0, 4) == 0 and args(INDEX, 0, 0, 5) == -1      # an index bit stays inside the row
    assert args(WORD, 0, 0, 63) == 0 and args(WORD, 0, 0, 64) == -1
    assert args(WORD, 1, 0, 0) == -1 and args(WORD, 0, 32, 0) == -1 and args(2, 0, 0, 0) == -1
