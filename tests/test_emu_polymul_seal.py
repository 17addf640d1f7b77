"""CPU emulation of the single-launch sealed negacyclic product (tests/emu/emu_polymul_seal.cpp compiles polymul_seal.hpp, the body of
k_polymul_mid_sealed cut at its barriers, with the very taps and pass templates the kernel instantiates): the words are the oracle's
product, the three digests are the seals of the host rows, a bit flipped in a factor moves exactly that factor's digest while all
three ABFT identities go on holding -- the gap the seal closes -- and the hooked tap moves the digest and not memory.  Without a GPU."""
import ctypes as C

import numpy as np
import pytest

from helpers.emu_build import build_emu
from helpers.sealed_case import py_seals
from oracle import cport as O

p64 = C.POINTER(C.c_uint64)
P = (1 << 61) - 1
GRID = [(logn, path, bits) for logn in (5, 10) for path, bits in ((0, 50), (1, 61))]


@pytest.fixture(scope="module")
def emu():
    L = build_emu("libemu_polymul_seal.so", ["emu_polymul_seal.cpp"], ("modarith.hpp", "ntt_core.hpp", "ntt_plan.hpp", "abft_taps.hpp", "seal_check.hpp",
                                                                       "ntt_seal_tap.hpp", "polymul_seal.hpp", "../../tests/emu/emu_ntt_seal.cpp"))
    L.emu_polymul_sealed.restype = C.c_int
    L.emu_polymul_sealed.argtypes = [p64, p64, p64, C.c_int, C.c_uint64, p64, p64, C.c_int, C.c_int, C.c_longlong, C.c_int, p64, p64]
    return L


class Case:
    """One (size, path): modulus, tables, the detector's weights, two clean rows in [16, q - 16), their product and the three
    seals, computed once."""

    def __init__(self, logn, path, bits):
        self.logn, self.path, self.N = logn, path, 1 << logn
        N = self.N
        self.q = q = int(O.gen_primes(N, bits, 1)[0])
        self.rp = np.ascontiguousarray(O.root_powers(q, logn), dtype=np.uint64)
        # w^ = F^-T w = N^-1 NTT(w_0, -w_{N-1}, ..., -w_1) in the engine's order (generate_weights, negaclic_ntt.py:7-13)
        p = 1 << (logn // 2)
        self.w = [((i % p + 1) + (i // p + 1)) % q for i in range(N)]
        u = np.array([self.w[0]] + [(q - self.w[N - i]) % q for i in range(1, N)], dtype=np.uint64)
        ninv = pow(N, -1, q)
        self.w_hat = np.array([int(v) * ninv % q for v in O.nwt_forward(u, q, self.rp)], dtype=np.uint64)
        rng = np.random.default_rng(500 * logn + path)
        self.a = rng.integers(16, q - 16, N, dtype=np.uint64)
        self.b = rng.integers(16, q - 16, N, dtype=np.uint64)
        self.psi = O.min_primitive_root(q, 2 * N)
        self.c = self.product(self.a, self.b)
        self.seals = [tuple(py_seals(v)[0]) for v in (self.a, self.b, self.c)]

    def product(self, a, b):
        """the oracle's negacyclic product of the rows as the unchecked product takes them: a word >= q reduced first"""
        q = np.uint64(self.q)
        return np.asarray(O.polymul_ntt(np.asarray(a) % q, np.asarray(b) % q, self.psi, self.q), dtype=np.uint64)

    def dot(self, x):
        return sum(w * int(v) for w, v in zip(self.w, x)) % self.q


_cases = {}


def case(logn, path, bits):
    if (logn, path) not in _cases:
        _cases[(logn, path)] = Case(logn, path, bits)
    return _cases[(logn, path)]


def canonical(s):
    return s % P


def run(emu, k, a, b, hit=(-1, 0, 0), alias=None):
    """(a after, b after, c, digests [(S0, S1) of a, b, c] canonical, (n_range a, n_range b), sums {ain, bin, aout, bout, cin, cout})"""
    a = np.ascontiguousarray(a, dtype=np.uint64).copy()
    b = np.ascontiguousarray(b, dtype=np.uint64).copy()
    c = a if alias == "a" else b if alias == "b" else np.zeros(k.N, dtype=np.uint64)
    parts, sums = np.zeros(8, dtype=np.uint64), np.zeros(6, dtype=np.uint64)
    rc = emu.emu_polymul_sealed(a.ctypes.data_as(p64), b.ctypes.data_as(p64), c.ctypes.data_as(p64), k.logn, k.q, k.rp.ctypes.data_as(p64),
                                k.w_hat.ctypes.data_as(p64), k.path, hit[0], hit[1], hit[2], parts.ctypes.data_as(p64), sums.ctypes.data_as(p64))
    assert rc == 0
    p = [int(v) for v in parts]
    dig = [(canonical(p[0]), canonical(p[1])), (canonical(p[3]), canonical(p[4])), (canonical(p[6]), canonical(p[7]))]
    return a, b, c, dig, (p[2], p[5]), [int(v) for v in sums]


def identities_hold(s):
    ain, bin_, aout, bout, cin, cout = s
    return ain == aout and bin_ == bout and cin == cout


@pytest.mark.parametrize("logn,path,bits", GRID)
def test_clean_product_words_digests_and_sums(emu, logn, path, bits):
    k = case(logn, path, bits)
    a, b, c, dig, nr, s = run(emu, k, k.a, k.b)
    assert (c == k.c).all()
    assert (a == k.a).all() and (b == k.b).all()          # the single launch only reads its factors
    assert dig == k.seals and nr == (0, 0)
    assert s[0] == k.dot(k.a) and s[1] == k.dot(k.b) and s[5] == k.dot(k.c)
    assert identities_hold(s)
    # c aliasing either factor: the same words and the same three digests
    for alias in ("a", "b"):
        _, _, c2, dig2, _, s2 = run(emu, k, k.a, k.b, alias=alias)
        assert (c2 == k.c).all() and dig2 == k.seals and s2 == s


@pytest.mark.parametrize("logn,path,bits", GRID)
def test_one_flipped_bit_moves_exactly_that_factors_digest_and_no_identity(emu, logn, path, bits):
    k = case(logn, path, bits)
    for op in (0, 1):
        for j, bit in ((0, 0), (k.N // 2 - 1, 40), (k.N // 2, 3), (k.N - 1, 63)):
            f = [k.a.copy(), k.b.copy()]
            f[op][j] ^= np.uint64(1 << bit)
            _, _, c, dig, nr, s = run(emu, k, f[0], f[1])
            assert dig[op] != k.seals[op] and dig[op] == tuple(py_seals(f[op])[0]), (op, j, bit)
            assert dig[1 - op] == k.seals[1 - op]
            assert (nr[op] == 1) == (int(f[op][j]) >= k.q) and nr[1 - op] == 0
            # the gap: the corrupted factor is a consistent input to all three identities, and every check passes on a wrong product
            assert identities_hold(s), (op, j, bit)
            want = k.product(f[0], f[1])
            assert (c == want).all() and not (c == k.c).all()
            assert dig[2] == tuple(py_seals(want)[0])       # the output digest is the seal of the words as stored


@pytest.mark.parametrize("logn,path,bits", GRID)
def test_hooked_tap_moves_the_digest_and_not_memory(emu, logn, path, bits):
    k = case(logn, path, bits)
    for op in (0, 1):
        for j, bit in ((0, 3), (k.N // 2 + 1, 40), (k.N - 1, 63)):
            a, b, c, dig, nr, s = run(emu, k, k.a, k.b, hit=(op, j, bit))
            assert (a == k.a).all() and (b == k.b).all()      # memory is untouched
            f = [k.a.copy(), k.b.copy()]
            f[op][j] ^= np.uint64(1 << bit)
            _, _, want, wdig, wnr, ws = run(emu, k, f[0], f[1])      # the same change made in memory
            assert (c == want).all() and dig == wdig and nr == wnr and s == ws
            assert dig[op] != k.seals[op] and dig[1 - op] == k.seals[1 - op]
