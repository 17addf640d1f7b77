"""CPU emulation of the ABFT detector's taps (tests/emu/emu_abft.cpp compiles abft_taps.hpp with the very same pass
templates the kernels instantiate): the checked inverse transform's two sums agree on a clean run and differ after a
flip between its launches, and the checked product's per-point sums satisfy sum w^ a^ b^ == sum w c against the
oracle's negacyclic product -- without a GPU."""
import ctypes as C

import numpy as np
import pytest

from helpers.emu_build import build_emu
from oracle import cport as O

p64 = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def emu():
    L = build_emu("libemu_abft.so", ["emu_abft.cpp"], ("modarith.hpp", "ntt_core.hpp", "ntt_plan.hpp", "abft_taps.hpp"))
    L.emu_inverse_checked.restype = C.c_int
    L.emu_inverse_checked.argtypes = [p64, C.c_int, C.c_uint64, p64, p64, C.c_int, C.c_longlong, C.c_int, p64]
    L.emu_product_sums.restype = C.c_int
    L.emu_product_sums.argtypes = [p64, p64, C.c_int, C.c_uint64, p64, p64, C.c_int, p64]
    return L


def _weights(logn, q):
    """w (generate_weights, negaclic_ntt.py:7-13) and w^ = F^-T w = N^-1 NTT(w_0, -w_{N-1}, ..., -w_1) in the engine's order."""
    N = 1 << logn
    p = 1 << (logn // 2)
    w = [((i % p + 1) + (i // p + 1)) % q for i in range(N)]
    u = np.array([w[0]] + [(q - w[N - i]) % q for i in range(1, N)], dtype=np.uint64)
    rp = O.root_powers(q, logn)
    ninv = pow(N, -1, q)
    w_hat = np.array([int(v) * ninv % q for v in O.nwt_forward(u, q, rp)], dtype=np.uint64)
    return w, w_hat, np.ascontiguousarray(rp, dtype=np.uint64)


def _dot(w, x, q):
    return sum(int(a) * int(b) for a, b in zip(w, x)) % q


def _inverse(emu, x, logn, q, rp, w_hat, path, flip=(-1, 0)):
    d = np.ascontiguousarray(x, dtype=np.uint64).copy()
    out = np.zeros(2, dtype=np.uint64)
    rc = emu.emu_inverse_checked(d.ctypes.data_as(p64), logn, q, rp.ctypes.data_as(p64), w_hat.ctypes.data_as(p64), path, flip[0], flip[1],
                                 out.ctypes.data_as(p64))
    assert rc == 0
    return d, int(out[0]), int(out[1])


@pytest.mark.parametrize("logn", [5, 8, 12, 13, 14, 16])
@pytest.mark.parametrize("path,bits", [(0, 50), (1, 61)])
def test_inverse_taps_agree_on_a_clean_run(emu, logn, path, bits):
    N = 1 << logn
    q = O.gen_primes(N, bits, 1)[0]
    w, w_hat, rp = _weights(logn, q)
    rng = np.random.default_rng(logn + path)
    x_hat = rng.integers(0, q, N, dtype=np.uint64)
    x, s_in, s_out = _inverse(emu, x_hat, logn, q, rp, w_hat, path)
    assert (x == O.nwt_inverse(x_hat, q, rp)).all()
    assert s_in == _dot(w_hat, x_hat, q)           # input side: w^ over the loaded words
    assert s_out == _dot(w, x, q)                  # output side: w over the stored words
    assert s_in == s_out


@pytest.mark.parametrize("logn", [13, 14, 16])
@pytest.mark.parametrize("path,bits", [(0, 50), (1, 61)])
def test_inverse_taps_disagree_after_a_flip_between_the_passes(emu, logn, path, bits):
    N = 1 << logn
    q = O.gen_primes(N, bits, 1)[0]
    w, w_hat, rp = _weights(logn, q)
    rng = np.random.default_rng(7 * logn + path)
    x_hat = rng.integers(0, q, N, dtype=np.uint64)
    x, s_in, s_out = _inverse(emu, x_hat, logn, q, rp, w_hat, path, flip=(int(rng.integers(0, N)), 30))
    assert s_in == _dot(w_hat, x_hat, q)
    assert s_out != s_in
    assert not (x == O.nwt_inverse(x_hat, q, rp)).all()


@pytest.mark.parametrize("logn", [5, 10, 14])
@pytest.mark.parametrize("path,bits", [(0, 50), (1, 61)])
def test_product_identity_against_oracle(emu, logn, path, bits):
    N = 1 << logn
    q = O.gen_primes(N, bits, 1)[0]
    w, w_hat, rp = _weights(logn, q)
    rng = np.random.default_rng(3 * logn + path)
    a = rng.integers(0, q, N, dtype=np.uint64)
    b = rng.integers(0, q, N, dtype=np.uint64)
    a[: N // 8] = q - 1                             # corner of the lazy ranges
    da, db = a.copy(), b.copy()
    out = np.zeros(5, dtype=np.uint64)
    rc = emu.emu_product_sums(da.ctypes.data_as(p64), db.ctypes.data_as(p64), logn, q, rp.ctypes.data_as(p64), w_hat.ctypes.data_as(p64), path,
                              out.ctypes.data_as(p64))
    assert rc == 0
    ain, bin_, aout, bout, cin = (int(v) for v in out)
    assert ain == _dot(w, a, q) and bin_ == _dot(w, b, q)
    assert aout == ain and bout == bin_              # forward checks of the two factors
    fa, fb = O.nwt_forward(a, q, rp), O.nwt_forward(b, q, rp)
    assert all(int(x) == int(y) * int(z) % q for x, y, z in zip(da, fa, fb))
    c = O.polymul_ntt(a, b, O.min_primitive_root(q, 2 * N), q)
    assert cin == _dot(w, c, q)                      # sum w^ a^ b^ == sum w c
