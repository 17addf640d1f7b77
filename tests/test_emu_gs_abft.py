"""CPU emulation of the checked natural-order (four-step) transform's taps (tests/emu/emu_gs_abft.cpp compiles GsTap of
abft_taps.hpp with the very same pass templates the kernels instantiate): on a clean run the output is the oracle's four-step
transform and the four sums -- sum u x over the gathered words, sum m z over the hand-off words as stored and as loaded, sum v y
over the stored words -- equal Python's dot products with weights computed here from their formulas, which pins the gathering
launch's index mapping and the hand-off layout; a flipped hand-off word breaks the hand-off identity and nothing else -- without
a GPU."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from helpers.emu_build import CSRC, build_emu
from oracle import cport as O

p64 = C.POINTER(C.c_uint64)

ROW_STAGES = {13: 8, 14: 8, 16: 8}          # P of the two-launch plans used here (ntt_plan.hpp): E2 = 2^P points, E1 = 2^(logN - P) columns
CASES = [("f64-ntt-prime", 0, 0), ("f64-50bit", 0, 50), ("u64-61bit", 1, 61)]


@pytest.fixture(scope="module")
def emu():
    # variation: two sources -- the library's own host_math.cpp is compiled in, since the emulation builds its tables with it
    L = build_emu("libemu_gs_abft.so", ["emu_gs_abft.cpp", os.path.join(CSRC, "host_math.cpp")],
                  ("host_math.hpp", "modarith.hpp", "ntt_core.hpp", "ntt_plan.hpp", "abft_taps.hpp"))
    L.emu_gs_checked.restype = C.c_int
    L.emu_gs_checked.argtypes = [p64, p64, C.c_int, C.c_uint64, C.c_uint64, p64, p64, p64, C.c_int, C.c_longlong, C.c_int, p64, p64]
    return L


def _modulus(logn, bits):
    """(q, g): 998244353 with its generator 3, or a prime of `bits` bits with N | q - 1 and a quadratic non-residue g, so that
    g^((q-1)/N) has order exactly N."""
    if not bits:
        return 998244353, 3
    q = O.gen_primes(1 << logn, bits, 1)[0]
    g = next(c for c in range(2, 1000) if pow(c, (q - 1) // 2, q) == q - 1)
    return q, g


def _brev(x, bits):
    return int(f"{x:0{bits}b}"[::-1], 2) if bits else 0


def _dft(a, w, q):
    """sum_j a[j] w^(i j) for every i, radix 2, Python integers."""
    n = len(a)
    if n == 1:
        return list(a)
    w2 = w * w % q
    e, o = _dft(a[0::2], w2, q), _dft(a[1::2], w2, q)
    out, t = [0] * n, 1
    for i in range(n // 2):
        x = t * o[i] % q
        out[i], out[i + n // 2] = (e[i] + x) % q, (e[i] - x) % q
        t = t * w % q
    return out


_WEIGHTS = {}


def _weights(logn, q, g):
    """v from its formula, u = W v through the oracle's four-step transform, m[c][k] = sum_j v[k + E2 j] (omega^(E2 c))^j at hand-off
    address brev(c) E2 + k (abft_taps.hpp)."""
    if (logn, q) in _WEIGHTS:
        return _WEIGHTS[(logn, q)]
    N, lp = 1 << logn, logn // 2
    v = [((i % (1 << lp)) + 1 + (i >> lp) + 1) % q for i in range(N)]
    u = [int(x) for x in O.four_step_ntt(np.array(v, dtype=np.uint64), 1 << lp, N >> lp, q, g)]
    m = None
    if logn in ROW_STAGES:
        P = ROW_STAGES[logn]
        S0 = logn - P
        E1, E2 = 1 << S0, 1 << P
        omega = pow(g, (q - 1) // N, q)
        m = [0] * N
        for k in range(E2):
            col = _dft([v[k + E2 * j] for j in range(E1)], pow(omega, E2, q), q)
            for c in range(E1):
                m[_brev(c, S0) * E2 + k] = col[c]
    _WEIGHTS[(logn, q)] = (u, m, v)
    return u, m, v


def _decode(word, path):
    """hand-off word -> the integer it stands for (FP64 path: raw double bits of an exact integer; integer path: the word)"""
    if path:
        return int(word)
    f = struct.unpack("<d", struct.pack("<Q", int(word)))[0]
    assert f == int(f), "hand-off word is not an integer"
    return int(f)


def _dot(w, x, q):
    return sum(int(a) * int(b) for a, b in zip(w, x)) % q


def _run(emu, x, logn, q, g, w3, path, flip=(-1, 0), inplace=False):
    u, m, v = (np.array(t if t is not None else [0] * len(x), dtype=np.uint64) for t in w3)
    src = np.ascontiguousarray(x, dtype=np.uint64).copy()
    dst = src if inplace else np.zeros_like(src)
    out = np.zeros(4, dtype=np.uint64)
    hand = np.zeros_like(src)
    rc = emu.emu_gs_checked(dst.ctypes.data_as(p64), src.ctypes.data_as(p64), logn, q, g, u.ctypes.data_as(p64), m.ctypes.data_as(p64), v.ctypes.data_as(p64), path,
                            flip[0], flip[1], out.ctypes.data_as(p64), hand.ctypes.data_as(p64))
    assert rc == 0
    return dst, [int(s) for s in out], hand


@pytest.mark.parametrize("logn", [5, 8, 12, 13, 14, 16])
@pytest.mark.parametrize("name,path,bits", CASES)
def test_clean_run_matches_the_oracle_and_python_sums(emu, logn, name, path, bits):
    N = 1 << logn
    q, g = _modulus(logn, bits)
    u, m, v = _weights(logn, q, g)
    assert sum(1 for t in (u, m, v) if t is not None for w in t if w % q == 0) == 0        # no blind word at these shapes
    rng = np.random.default_rng(100 * logn + path + bits)
    x = rng.integers(0, q, N, dtype=np.uint64)
    x[: N // 8] = q - 1                             # corner of the lazy ranges
    want = O.four_step_ntt(x, 1 << (logn // 2), N >> (logn // 2), q, g)
    for inplace in (False, True):
        y, s, hand = _run(emu, x, logn, q, g, (u, m, v), path, inplace=inplace)
        assert (y == want).all()
        assert s[0] == _dot(u, x, q)                # gathered words at their natural source index
        assert s[3] == _dot(v, want, q)
        if m is None:
            assert s[0] == s[3]
        else:
            z = [_decode(w, path) for w in hand]
            assert s[1] == _dot(m, z, q) and s[2] == s[1]      # hand-off layout
            assert s[0] == s[1] == s[2] == s[3]


@pytest.mark.parametrize("logn", [13, 14, 16])
@pytest.mark.parametrize("name,path,bits", CASES)
def test_flipped_handoff_word_breaks_the_handoff_identity_only(emu, logn, name, path, bits):
    N = 1 << logn
    q, g = _modulus(logn, bits)
    u, m, v = _weights(logn, q, g)
    rng = np.random.default_rng(7 * logn + path + bits)
    x = rng.integers(0, q, N, dtype=np.uint64)
    y0, s0, hand = _run(emu, x, logn, q, g, (u, m, v), path)
    # FP64 words: the sign and the two top mantissa bits keep the word an integer; integer path: bits that keep it below 2q
    pairs = [(0, 63), (N - 1, 51), (N // 2 + 1, 50), (12345 % N, 63), (N // 3, 51)] if path == 0 else [(0, 0), (N - 1, 40), (N // 2 + 1, 17), (12345 % N, 59), (N // 3, 33)]
    for word, bit in pairs:
        while True:                                  # the first word from there on whose flipped form the arithmetic accepts
            flipped = int(hand[word]) ^ (1 << bit)
            if path == 0:
                ok = abs(_decode(hand[word], path)) >= 4
            else:
                ok = flipped < 2 * q
            if ok:
                break
            word = (word + 1) % N
        y, s, _ = _run(emu, x, logn, q, g, (u, m, v), path, flip=(word, bit))
        z = [_decode(w, path) for w in hand]
        z[word] = _decode(flipped, path)
        assert s[0] == s0[0] and s[1] == s0[1] and s[0] == s[1]     # launch 1 untouched
        assert s[2] == _dot(m, z, q)                                   # launch 2 weighs what it loaded
        assert s[2] != s[1]                                            # hand-off identity broken
        assert s[3] == s[2]                                            # launch-2 identity holds on the corrupted data
        assert (y != y0).any()
