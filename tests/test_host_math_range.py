"""The host number theory behind the C ABI across the whole modulus range (no GPU needed): fhe_moduli_create, fhe_min_primitive_root,
fhe_modulus_const_ratio and fhe_root_powers against tests/helpers/number_theory.py -- Python integers, trial division and
Miller-Rabin by ``pow`` -- from the 2-bit primes to the 61-bit ones, on both sides of the path switch at 2^50, at the smallest prime
that exists for a transform size, and at every argument the header says is refused."""
import ctypes as C
import random
import subprocess
import sys
import time

import numpy as np
import pytest

from helpers import number_theory as NT

ERR_INVALID, ERR_UNSUPPORTED = 1, 3
SIZES = [2, 1 << 4, 1 << 10, 1 << 15, 1 << 17, 1 << 20]
MAX_ORDER = 1 << 31                       # include/fhe_mi355x.h, fhe_min_primitive_root


@pytest.fixture(scope="module")
def lib():
    from fhe_reliability_gpu_amd._lib import lib as L
    return L


def _moduli(lib, N, bits):
    out = (C.c_uint64 * max(len(bits), 1))()
    rc = lib.fhe_moduli_create(C.c_uint64(N), (C.c_int * max(len(bits), 1))(*bits), len(bits), out)
    return rc, [int(x) for x in out][:len(bits)]


def _root(lib, q, order):
    out = C.c_uint64(0)
    rc = lib.fhe_min_primitive_root(C.c_uint64(q), C.c_uint64(order), C.byref(out))
    return rc, int(out.value)


def around_2_50(N):
    """the last prime below 2^50 and the first above it that are 1 mod 2N"""
    return NT.last_prime_below(1 << 50, N), NT.first_prime_above(1 << 50, N)


# ------------------------------------------------------------------ the reference itself, where an independent statement exists
def test_reference_primality_agrees_with_a_sieve_and_rejects_pseudoprimes():
    limit = 1 << 16
    sieve = bytearray([1]) * limit
    sieve[0] = sieve[1] = 0
    for i in range(2, 256):
        if sieve[i]:
            sieve[i * i::i] = bytearray(len(range(i * i, limit, i)))
    assert [n for n in range(limit) if NT.is_prime(n)] == [n for n in range(limit) if sieve[n]]
    # strong pseudoprimes to base 2, Carmichael numbers, and products of two primes next to 2^25 and 2^30 (Miller-Rabin's side)
    for n in (2047, 3277, 4033, 561, 1105, 1729, 41041, 825265, 3215031751, 33554393 * 33554467, 1073741789 * 1073741827):
        assert not NT.is_prime(n)
    for p in (1048583, 2305843009213693951, 1125899903107073, 2305843009211596801, 18446744073709551557):
        assert NT.is_prime(p)


def test_reference_transform_and_product_match_the_oracle():
    """the schoolbook forms at 2^4 and 2^6 pin the oracle that stands in for them at the larger sizes"""
    from oracle import cport as O
    rng = random.Random(5)
    for logn in (4, 6):
        N = 1 << logn
        lo, hi = around_2_50(N)
        for q in (NT.smallest_prime(N), lo, hi):
            psi = NT.min_primitive_root(q, 2 * N)
            assert psi == O.min_primitive_root(q, 2 * N)
            rp, sh = NT.root_powers(q, logn, psi)
            orp, osh = O.root_powers(q, logn, psi, shoup=True)
            assert rp == [int(x) for x in orp] and sh == [int(x) for x in osh]
            a, b = ([rng.randrange(q) for _ in range(N)] for _ in range(2))
            fa = NT.negacyclic_forward(a, q, psi)
            assert fa == [int(x) for x in O.nwt_forward(a, q, orp)]
            assert NT.negacyclic_inverse(fa, q, psi) == a == [int(x) for x in O.nwt_inverse(fa, q, orp)]
            c = NT.negacyclic_product(a, b, q)
            assert c == [int(x) for x in O.polymul_ntt(a, b, psi, q)] == [int(x) for x in O.polymul_naive(a, b, q)]


def test_reference_cyclic_table_runs_the_transform():
    """the table of cyclic_table's comment, in both conventions, drives the decimation-in-frequency network (stage by stage from
    the whole length down, block b of a stage of 2m blocks' worth of factors reads tw[m + b]) to the DFT in bit-reversed order"""
    for mod, g, logn in ((97, 5, 4), (12289, 11, 5), (998244353, 3, 6)):
        n = 1 << logn
        w = pow(g, (mod - 1) // n, mod)
        assert pow(w, n // 2, mod) == mod - 1
        tables = [NT.cyclic_table(mod, logn, g, False), NT.cyclic_table(mod, logn, w, True)]
        assert tables[0] == tables[1] and tables[0][0] == 1
        tw = tables[0]
        rng = random.Random(logn)
        x = [rng.randrange(mod) for _ in range(n)]
        a = list(x)
        for s in range(logn):                        # Cooley-Tukey on bit-reversed factors: 2^s blocks, partner half a block away
            m, t = 1 << s, n >> (s + 1)
            for b in range(m):
                for j in range(b * 2 * t, b * 2 * t + t):
                    u, v = a[j], a[j + t] * tw[m + b] % mod
                    a[j], a[j + t] = (u + v) % mod, (u - v) % mod
        want = [sum(x[i] * pow(w, i * k, mod) for i in range(n)) % mod for k in range(n)]
        assert a == [want[NT.bit_reverse(k, logn)] for k in range(n)]


# ------------------------------------------------------------------ fhe_moduli_create
@pytest.mark.parametrize("bits", range(2, 17))
def test_every_prime_of_an_interval(lib, bits):
    """N = 1: every odd number of (2^(bits-1), 2^bits) is a candidate, 2047, 3277, 4033 and the Carmichael numbers among them"""
    want = NT.primes_in_class(1, bits)
    rc, got = _moduli(lib, 1, [bits] * len(want))
    assert rc == 0 and got == want
    rc, _ = _moduli(lib, 1, [bits] * (len(want) + 1))
    assert rc != 0


@pytest.mark.parametrize("N", SIZES)
def test_three_primes_of_every_size(lib, N):
    for bits in range(17, 62):
        try:
            want = NT.primes_in_class(N, bits, 3)
        except ValueError:
            want = None
        rc, got = _moduli(lib, N, [bits] * 3)
        if want is None:
            assert rc != 0, (N, bits, got)
        else:
            assert rc == 0 and got == want, (N, bits)
    assert _moduli(lib, 1 << 20, [22] * 3)[0] != 0           # (2^21, 2^22) holds one candidate: 2^21 + 1 = 3 x 699051


def test_mixed_request_order(lib):
    bits = [50, 61, 50, 61, 50, 30, 61]
    for N in (1 << 12, 1 << 16):
        rc, got = _moduli(lib, N, bits)
        assert rc == 0 and got == NT.create_moduli(N, bits)
        p50, p61 = NT.primes_in_class(N, 50, 3), NT.primes_in_class(N, 61, 3)
        assert got == [p50[0], p61[0], p50[1], p61[1], p50[2], NT.primes_in_class(N, 30, 1)[0], p61[2]]


def test_moduli_refusals(lib):
    for bits in (1, 62, 0, -1):
        assert _moduli(lib, 1 << 10, [bits])[0] == ERR_UNSUPPORTED
        assert _moduli(lib, 1 << 10, [50, bits])[0] == ERR_UNSUPPORTED
    assert _moduli(lib, 1 << 10, [])[0] == ERR_INVALID
    out = (C.c_uint64 * 1)()
    assert lib.fhe_moduli_create(C.c_uint64(1 << 10), (C.c_int * 1)(50), -1, out) == ERR_INVALID
    for N in (0, 3, 1 << 60, 1 << 61, 1 << 62):
        for bits in (2, 50, 61):
            assert _moduli(lib, N, [bits])[0] == ERR_INVALID, (N, bits)
    # the largest N the header admits: accepted as an argument, and no prime of at most 61 bits is 1 mod 2^60 (2^60 + 1 = 17 x ..)
    assert _moduli(lib, 1 << 59, [61])[0] == ERR_INVALID and not NT.is_prime((1 << 60) + 1)
    rc, got = _moduli(lib, 1 << 55, [61])                      # 27 x 2^56 + 1, the only prime of its class
    assert rc == 0 and got == NT.primes_in_class(1 << 55, 61) == [27 * 2**56 + 1]
    assert lib.fhe_last_error()


def test_moduli_n_2_63_returns_a_status():
    """2 N wraps to 0 in 64 bits: the call must come back with a status (in a child process, so that a division by zero there
    ends the child and not this run)"""
    code = ("import ctypes as C\n"
            "from fhe_reliability_gpu_amd._lib import lib\n"
            "out = (C.c_uint64 * 1)()\n"
            "for bits in (2, 50, 61):\n"
            "    rc = lib.fhe_moduli_create(C.c_uint64(1 << 63), (C.c_int * 1)(bits), 1, out)\n"
            "    assert rc == 1, rc\n"
            "print('status', rc)\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "status 1", (r.returncode, r.stdout, r.stderr[-400:])


# ------------------------------------------------------------------ fhe_min_primitive_root
def test_roots_of_every_prime_below_2000(lib):
    n = 0
    for q in range(3, 2000):
        if not NT.is_prime(q):
            continue
        order = 2
        while (q - 1) % order == 0:
            rc, got = _root(lib, q, order)
            assert rc == 0 and got == NT.min_primitive_root(q, order), (q, order)
            if order == 2:
                assert got == q - 1
            order *= 2
            n += 1
        assert _root(lib, q, order)[0] == ERR_INVALID          # the first power of two that does not divide q - 1
    assert n > 500
    for q, order in ((3, 2), (17, 16), (97, 32), (12289, 4096), (40961, 8192), (65537, 65536)):
        assert _root(lib, q, order) == (0, NT.min_primitive_root(q, order))
    # (by hand: 2 = -1 mod 3; 2 has order 8 modulo 17 and 3 is a generator; 3 generates the units of the Fermat prime 65537)
    assert [NT.min_primitive_root(q, o) for q, o in ((3, 2), (17, 16), (65537, 65536))] == [2, 3, 3]


def test_order_two_gives_q_minus_one(lib):
    for N in (1 << 4, 1 << 16):
        for q in (NT.smallest_prime(N), *around_2_50(N), NT.primes_in_class(N, 61, 1)[0], NT.primes_in_class(N, 30, 1)[0]):
            assert _root(lib, q, 2) == (0, q - 1)


@pytest.mark.parametrize("logn", range(1, 17))
def test_roots_of_the_smallest_prime_of_every_size(lib, logn):
    q = NT.smallest_prime(1 << logn)
    for order in sorted({2 << logn, 1 << logn, 4}):
        assert _root(lib, q, order) == (0, NT.min_primitive_root(q, order)), (q, order)


@pytest.mark.parametrize("order", [1 << 5, 1 << 14, 1 << 18])
def test_roots_around_2_50_and_at_the_top(lib, order):
    lo, hi = around_2_50(order // 2)
    assert lo < 1 << 50 < hi
    for q in (lo, hi, NT.primes_in_class(order // 2, 61, 1)[0]):
        assert _root(lib, q, order) == (0, NT.min_primitive_root(q, order)), (q, order)


def test_root_refusals(lib):
    t = time.perf_counter()
    assert lib.fhe_min_primitive_root(C.c_uint64(97), C.c_uint64(32), None) == ERR_INVALID
    for q, order in ((97, 0), (97, 1), (97, 3), (97, 6), (97, 24), (97, 64), (12289, 8192), (0, 2), (1, 2), (2, 2), (0, 1 << 10), (1, 1 << 10),
                     (2, 1 << 10)):
        assert _root(lib, q, order)[0] == ERR_INVALID, (q, order)
    # composites that are 1 mod the order, strong pseudoprimes to base 2 and Carmichael numbers among them
    for q, order in ((2047, 2), (3277, 4), (4033, 64), (561, 16), (1729, 64), (41041, 16), (15, 2), (65, 64), (85, 4), ((1 << 32) + 1, 1 << 27),
                     (1073741789 * 1073741827, 2), ((1 << 50) - 1, 2), (12289 * 40961, 4096)):
        assert (q - 1) % order == 0 and not NT.is_prime(q)
        assert _root(lib, q, order)[0] == ERR_INVALID, (q, order)
    assert time.perf_counter() - t < 2.0


def test_largest_order(lib):
    """2^31 is the largest order taken (fhe_root_powers' log_n = 30); the search walks order / 2 products, so one order above is
    refused by its size, at once, although the prime has such a subgroup"""
    q = NT.smallest_prime(1 << 39)                 # 1 mod 2^40
    assert (q - 1) % (1 << 40) == 0 and q < 1 << 61
    t = time.perf_counter()
    for order in (MAX_ORDER << 1, 1 << 40):
        assert _root(lib, q, order)[0] == ERR_UNSUPPORTED
    assert time.perf_counter() - t < 1.0
    assert _root(lib, q, 1 << 20) == (0, NT.min_primitive_root(q, 1 << 20))


# ------------------------------------------------------------------ fhe_modulus_const_ratio
def test_const_ratio(lib):
    qs = [2, 3, 4, 2**64 - 1]
    for k in (8, 31, 32, 33, 50, 61, 63):
        qs += [2**k - 1, 2**k, 2**k + 1]
    for N in (1 << 4, 1 << 16):
        qs += [NT.primes_in_class(N, 30, 1)[0], *around_2_50(N), NT.primes_in_class(N, 61, 1)[0]]
    assert any(q.bit_length() == 51 and NT.is_prime(q) for q in qs)
    rng = random.Random(128)
    qs += [rng.getrandbits(64) | (1 << 63) for _ in range(500)] + [rng.randrange(2, 2**64) for _ in range(500)]
    r = (C.c_uint64 * 3)()
    for q in qs:
        assert lib.fhe_modulus_const_ratio(C.c_uint64(q), r) == 0
        assert [int(x) for x in r] == NT.const_ratio(q), q
    for q in (0, 1):
        assert lib.fhe_modulus_const_ratio(C.c_uint64(q), r) == ERR_INVALID
    assert lib.fhe_modulus_const_ratio(C.c_uint64(97), None) == ERR_INVALID


# ------------------------------------------------------------------ fhe_root_powers
def _root_powers(lib, q, logn, want_rp=True, want_shoup=True):
    N = 1 << logn
    rp, sh = np.full(N, 0x5E5E5E5E5E5E5E5E, dtype=np.uint64), np.full(N, 0x5E5E5E5E5E5E5E5E, dtype=np.uint64)
    p = lambda a, on: a.ctypes.data_as(C.POINTER(C.c_uint64)) if on else None
    rc = lib.fhe_root_powers(C.c_uint64(q), logn, p(rp, want_rp), p(sh, want_shoup))
    return rc, [int(x) for x in rp], [int(x) for x in sh]


@pytest.mark.parametrize("logn", range(1, 13))
def test_root_powers_and_shoup_words(lib, logn):
    N = 1 << logn
    for q in (NT.smallest_prime(N), NT.primes_in_class(N, 30, 1)[0], *around_2_50(N), NT.primes_in_class(N, 61, 1)[0]):
        psi = NT.min_primitive_root(q, 2 * N)
        want_rp, want_sh = NT.root_powers(q, logn, psi)
        assert _root_powers(lib, q, logn) == (0, want_rp, want_sh), q
        untouched = [0x5E5E5E5E5E5E5E5E] * N
        assert _root_powers(lib, q, logn, want_shoup=False) == (0, want_rp, untouched), q
        assert _root_powers(lib, q, logn, want_rp=False) == (0, untouched, want_sh), q
        assert _root_powers(lib, q, logn, False, False)[0] == 0
        assert want_rp[0] == 1 and want_rp[1] == pow(psi, N // 2, q) and pow(want_rp[1], 2, q) == q - 1


def test_root_powers_refusals(lib):
    q = 40961                                                     # 5 x 2^13 + 1
    assert NT.is_prime(q) and (q - 1) % (1 << 13) == 0 and (q - 1) % (1 << 14) != 0
    assert _root_powers(lib, q, 12)[0] == 0
    t = time.perf_counter()
    for logn in (0, -1, 31, 13):                                  # 13: q is not 1 mod 2N
        assert lib.fhe_root_powers(C.c_uint64(q), logn, None, None) == ERR_INVALID, logn
    composite = next(c for c in range((1 << 13) + 1, 1 << 20, 1 << 13) if not NT.is_prime(c))          # 1 mod 2N, not prime
    for bad in (0, 1, 2, composite, (1 << 50) - 1, 12289 * 40961):
        assert lib.fhe_root_powers(C.c_uint64(bad), 12, None, None) == ERR_INVALID, bad
    assert time.perf_counter() - t < 2.0
