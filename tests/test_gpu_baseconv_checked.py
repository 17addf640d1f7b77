"""Residue-checked base conversions on the device (baseconv_checked.hip): fhe_baseconv_exact_checked / _fast_checked give
the unchecked calls' words bit for bit with every flag clear on clean runs, flag exactly the unit a hook fault hit (and only
when the fault changed an output word), and raise only bit 4 on an input word that is not canonical."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import cport as O

pytestmark = pytest.mark.gpu

RESIDUE, RANGE, OPERAND = 1, 2, 4
PRODUCT, QUOTIENT, RESULT, SUM = 0, 1, 2, 3
ERR_INVALID, ERR_UNSUPPORTED = 1, 3
GARBAGE = 0xA5A5A5A5DEADBEEF
SENTINEL = 0x5E5E5E5E5E5E5E5E
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "baseconv.json")


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


@pytest.fixture(scope="module")
def L():
    from fhe_reliability_gpu_amd._lib import lib
    return lib


def _flags_buf(eng, n):
    """a flags buffer pre-filled with garbage: the call must clear it"""
    return eng.upload(np.full((n + 1) // 2, GARBAGE, dtype=np.uint64))


def _read_flags(buf, n):
    return buf.download().view(np.uint32)[:n].copy()


def _rand(rng, mi, N):
    x = np.stack([rng.integers(0, p, N, dtype=np.uint64) for p in mi])
    for j, p in enumerate(mi):                      # edge words
        x[j, 0], x[j, 1 % N] = 0, p - 1
    return x


def _checked(eng, L, bc, x, N, exact=True, stream=None, out=None):
    """-> rc, words [k][N], flags"""
    units = bc.m + bc.k if exact else bc.k
    d_in = eng.upload(x)
    d_out = out if out is not None else eng.alloc(bc.k * N)
    flags = _flags_buf(eng, units)
    f = L.fhe_baseconv_exact_checked if exact else L.fhe_baseconv_fast_checked
    rc = f(eng._h, d_out.ptr, d_in.ptr, bc._h, N, flags.ptr, stream)
    if stream is not None:
        eng.sync(stream)
    return rc, d_out.download().reshape(bc.k, N), _read_flags(flags, units)


def _plain(eng, bc, x, N, exact=True):
    d_in, d_out = eng.upload(x), eng.alloc(bc.k * N)
    (bc.exact if exact else bc.fast)(d_out, d_in, N)
    return d_out.download().reshape(bc.k, N)


def _oracle(mi, mo, x, exact, cols=None):
    """oracle/cport.py on all columns or a sample of them, [k][columns]"""
    xs = np.ascontiguousarray(x if cols is None else x[:, cols])
    return O.baseconv_exact(xs, mi, mo) if exact else O.bconv_fast(xs, mi, mo).T


def _clean_case(F, eng, L, mi, mo, x, N, exact, seed=0):
    bc = F.BaseConv(eng, mi, mo)
    rc, got, flags = _checked(eng, L, bc, x, N, exact)
    assert rc == 0
    assert not flags.any(), flags
    assert (got == _plain(eng, bc, x, N, exact)).all()
    cols = None if N <= 1 << 12 else np.random.default_rng(seed).integers(0, N, 64)
    want = _oracle(mi, mo, x, exact, cols)
    assert ((got if cols is None else got[:, cols]) == want).all()


@pytest.mark.parametrize("case", ["exact", "exact50", "fast", "fast31"])
def test_golden_case(F, eng, L, case):
    with open(GOLDEN) as fh:
        g = json.load(fh)[case]
    mi, mo = g["mod_in"], g["mod_out"]
    x = np.array(g["res"], dtype=np.uint64)
    N = x.shape[1]
    exact = case.startswith("exact")
    want = np.array(g["out"], dtype=np.uint64)
    want = want if exact else want.T
    bc = F.BaseConv(eng, mi, mo)
    rc, got, flags = _checked(eng, L, bc, x, N, exact)
    assert rc == 0 and not flags.any()
    assert (got == want).all()
    assert (got == _plain(eng, bc, x, N, exact)).all()


def _moduli(F, N, m, k, big):
    """m + k distinct primes: all 50 bits (FP64 plan), or with one 61-bit prime among the inputs (integer plan)"""
    qs = F.create_moduli(N, [50] * (m + k - 1) + [61 if big else 50])
    qs = qs[-1:] + qs[:-1] if big else qs
    return qs[:m], qs[m:]


@pytest.mark.parametrize("m,k", [(1, 1), (4, 8), (16, 16), (17, 5), (40, 24)])
@pytest.mark.parametrize("big", [False, True])
def test_exact_checked_clean_small(F, eng, L, m, k, big):
    N = 1 << 10
    mi, mo = _moduli(F, N, m, k, big)
    _clean_case(F, eng, L, mi, mo, _rand(np.random.default_rng(m * 64 + k), mi, N), N, True)


@pytest.mark.parametrize("logn,m,k", [(16, 11, 44), (17, 8, 32)])
@pytest.mark.parametrize("big", [False, True])
def test_exact_checked_clean_keyswitch_shapes(F, eng, L, logn, m, k, big):
    N = 1 << logn
    mi, mo = _moduli(F, N, m, k, big)
    _clean_case(F, eng, L, mi, mo, _rand(np.random.default_rng(logn + big), mi, N), N, True, seed=logn)


@pytest.mark.parametrize("N", [2, 1000])
@pytest.mark.parametrize("big", [False, True])
def test_checked_clean_odd_sizes(F, eng, L, N, big):
    mi, mo = _moduli(F, 1 << 10, 5, 7, big)
    x = _rand(np.random.default_rng(N), mi, N)
    _clean_case(F, eng, L, mi, mo, x, N, True)
    if not big:
        _clean_case(F, eng, L, mi, mo, x, N, False)


@pytest.mark.parametrize("m,k,logn", [(1, 1, 10), (4, 8, 10), (16, 16, 10), (40, 24, 10), (8, 32, 17)])
def test_fast_checked_clean(F, eng, L, m, k, logn):
    N = 1 << logn
    mi, mo = _moduli(F, N, m, k, False)
    _clean_case(F, eng, L, mi, mo, _rand(np.random.default_rng(m + k), mi, N), N, False, seed=m)


def test_fast_checked_clean_61_bit_output(F, eng, L):
    N = 1 << 10
    qs = F.create_moduli(N, [50, 50, 50, 61, 61])
    mi, mo = qs[:3], qs[3:]
    _clean_case(F, eng, L, mi, mo, _rand(np.random.default_rng(4), mi, N), N, False)


# ---- the test hook -----------------------------------------------------------------------------------------------------
def _arm(eng, L, point, unit, coeff, bit):
    return L.fhe_ctx_inject_fault_baseconv(eng._h, point, unit, coeff, bit)


def _hook_sweep(F, eng, L, mi, mo, exact, units, N):
    m, k = len(mi), len(mo)
    bc = F.BaseConv(eng, mi, mo)
    x = _rand(np.random.default_rng(41 + exact), mi, N)
    rc, clean, flags = _checked(eng, L, bc, x, N, exact)
    assert rc == 0 and not flags.any()
    seen_changed = 0
    for unit in units:
        terms = (unit + 1 if unit < m else m) if exact else m
        points = [PRODUCT, QUOTIENT, RESULT] + ([SUM] if terms >= 2 else [])
        for point in points:
            for bit in (0, 5, 31, 47, 63, 1):
                coeff = (bit * 37 + unit * 101 + point) % N
                assert _arm(eng, L, point, unit, coeff, bit) == 0
                rc, got, f = _checked(eng, L, bc, x, N, exact)
                assert rc == 0
                cols = np.nonzero((got != clean).any(axis=0))[0]
                assert set(cols.tolist()) <= {coeff}, f"unit {unit} point {point} bit {bit}: another coefficient changed"
                changed = cols.size > 0
                seen_changed += changed
                assert not np.delete(f, unit).any(), f"unit {unit} point {point} bit {bit}: flags {f}"
                assert bool(f[unit]) == changed, f"unit {unit} point {point} bit {bit}: changed {changed}, flags {f[unit]}"
                assert not (f[unit] & OPERAND)
                if not exact or unit >= m:          # an output fault touches that output's word alone
                    o = unit - m if exact else unit
                    assert (np.delete(got, o, axis=0) == np.delete(clean, o, axis=0)).all()
        # one shot: the next call is clean
        rc, got, f = _checked(eng, L, bc, x, N, exact)
        assert rc == 0 and not f.any() and (got == clean).all()
    assert seen_changed >= 3 * len(units)


@pytest.mark.parametrize("big", [False, True])
def test_exact_hook_flags_exactly_the_unit_it_hit(F, eng, L, big):
    N = 1 << 10
    mi, mo = _moduli(F, N, 4, 6, big)
    _hook_sweep(F, eng, L, mi, mo, True, [0, 2, 3, 4 + 0, 4 + 5], N)


def test_exact_hook_on_sliced_and_runtime_m_launches(F, eng, L):
    # N = 256: one workgroup per output slice, so the outputs are cut over workgroups that each recompute the digits;
    # m = 17: the runtime-m kernel
    N = 256
    mi, mo = _moduli(F, 1 << 10, 3, 16, False)
    _hook_sweep(F, eng, L, mi, mo, True, [1, 3 + 15], N)
    mi, mo = _moduli(F, 1 << 10, 17, 4, True)
    _hook_sweep(F, eng, L, mi, mo, True, [16, 17 + 3], N)


@pytest.mark.parametrize("bits", [50, 61])
def test_fast_hook_flags_exactly_the_unit_it_hit(F, eng, L, bits):
    N = 1 << 10
    qs = F.create_moduli(N, [50] * 4 + [bits] * 6)
    _hook_sweep(F, eng, L, qs[:4], qs[4:], False, [0, 5], N)


@pytest.mark.parametrize("big", [False, True])
def test_noncanonical_input_raises_bit_4_on_its_digit_only(F, eng, L, big):
    N = 1 << 11
    m, k = 5, 6
    mi, mo = _moduli(F, N, m, k, big)
    bc = F.BaseConv(eng, mi, mo)
    x = _rand(np.random.default_rng(9 + big), mi, N)
    x[0, 300] = np.uint64(2**64 - 1)
    x[3, 7] = np.uint64(mi[3])                       # exactly p_j
    x[3, 1999] = np.uint64(mi[3] + 12345)
    rc, got, f = _checked(eng, L, bc, x, N, True)
    assert rc == 0
    want = np.zeros(m + k, dtype=np.uint32)
    want[0] = want[3] = OPERAND
    assert (f == want).all()
    assert (got == _plain(eng, bc, x, N, True)).all()
    assert (got == O.baseconv_exact(x % np.array(mi, dtype=np.uint64)[:, None], mi, mo)).all()
    if not big:
        # the fast form takes any word and flags nothing
        rc, got, f = _checked(eng, L, bc, x, N, False)
        assert rc == 0 and not f.any()
        assert (got == _plain(eng, bc, x, N, False)).all()


def test_statuses(F, eng, L):
    N = 1 << 10
    m, k = 4, 6
    mi, mo = _moduli(F, N, m, k, False)
    bc = F.BaseConv(eng, mi, mo)
    x = _rand(np.random.default_rng(1), mi, N)
    d_in, flags = eng.upload(x), _flags_buf(eng, m + k)
    sentinel = np.full(k * N, SENTINEL, dtype=np.uint64)
    d_out = eng.upload(sentinel)
    for f in (L.fhe_baseconv_exact_checked, L.fhe_baseconv_fast_checked):
        assert f(eng._h, d_out.ptr, d_in.ptr, bc._h, N, None, None) == ERR_INVALID           # null flags
        assert f(eng._h, d_out.ptr, d_in.ptr, None, N, flags.ptr, None) == ERR_INVALID       # null plan
        assert f(eng._h, None, d_in.ptr, bc._h, N, flags.ptr, None) == ERR_INVALID
    assert _arm(eng, L, 4, 0, 0, 0) == ERR_INVALID
    assert _arm(eng, L, 0, 0, 0, 64) == ERR_INVALID
    assert _arm(eng, L, 0, -1, 0, 0) == ERR_INVALID
    assert _arm(eng, L, 0, 0, -1, 0) == ERR_INVALID
    assert _arm(eng, L, -1, 0, 0, 0) == 0
    # faults that do not exist for the call: a status, nothing launched, the hook used up
    for arm, exact, want in (((PRODUCT, m + k, 0, 0), True, ERR_INVALID),       # unit outside the call
                             ((PRODUCT, 0, N, 0), True, ERR_INVALID),           # coefficient outside the call
                             ((SUM, 0, 5, 3), True, ERR_UNSUPPORTED),           # digit 0 is a one-term sum
                             ((PRODUCT, k, 0, 0), False, ERR_INVALID)):
        assert _arm(eng, L, *arm) == 0
        f = L.fhe_baseconv_exact_checked if exact else L.fhe_baseconv_fast_checked
        assert f(eng._h, d_out.ptr, d_in.ptr, bc._h, N, flags.ptr, None) == want
        eng.sync()
        assert (d_out.download() == sentinel).all()
        rc, got, fl = _checked(eng, L, bc, x, N, exact)
        assert rc == 0 and not fl.any() and (got == _plain(eng, bc, x, N, exact)).all()
    # a one-limb base has no running sum on its outputs either
    one = F.BaseConv(eng, mi[:1], mo)
    assert _arm(eng, L, SUM, 1, 0, 0) == 0
    assert L.fhe_baseconv_exact_checked(eng._h, d_out.ptr, d_in.ptr, one._h, N, flags.ptr, None) == ERR_UNSUPPORTED
    assert _arm(eng, L, SUM, 0, 0, 0) == 0
    assert L.fhe_baseconv_fast_checked(eng._h, d_out.ptr, d_in.ptr, one._h, N, flags.ptr, None) == ERR_UNSUPPORTED
    eng.sync()
    assert (d_out.download() == sentinel).all()
    # the fast form on a plan whose unreduced sum would pass 64 bits
    qs = F.create_moduli(N, [61] * 17)            # 16 terms of at least 2^60
    wide = F.BaseConv(eng, qs[:16], qs[16:])
    d8 = eng.upload(_rand(np.random.default_rng(2), qs[:16], N))
    assert L.fhe_baseconv_fast(eng._h, d_out.ptr, d8.ptr, wide._h, N, None) == ERR_UNSUPPORTED
    assert L.fhe_baseconv_fast_checked(eng._h, d_out.ptr, d8.ptr, wide._h, N, flags.ptr, None) == ERR_UNSUPPORTED
    eng.sync()
    assert (d_out.download() == sentinel).all()


def test_python_wrappers(F, eng):
    N = 1 << 10
    m, k = 3, 5
    mi, mo = _moduli(F, N, m, k, False)
    bc = F.BaseConv(eng, mi, mo)
    x = _rand(np.random.default_rng(6), mi, N)
    d_in, d_out = eng.upload(x), eng.alloc(k * N)
    f = bc.exact_checked(d_out, d_in, N)
    assert f.dtype == np.uint32 and f.shape == (m + k,) and not f.any()
    assert (d_out.download().reshape(k, N) == O.baseconv_exact(x, mi, mo)).all()
    f = bc.fast_checked(d_out, d_in, N)
    assert f.dtype == np.uint32 and f.shape == (k,) and not f.any()
    assert (d_out.download().reshape(k, N) == O.bconv_fast(x, mi, mo).T).all()


def test_two_streams_with_separate_flag_buffers(F, eng, L):
    import torch
    N = 1 << 14
    m, k = 8, 12
    mi, mo = _moduli(F, N, m, k, False)
    bc = F.BaseConv(eng, mi, mo)
    rng = np.random.default_rng(8)
    xs = [_rand(rng, mi, N) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    d_in = [eng.upload(x) for x in xs]
    d_out = [eng.alloc(k * N) for _ in range(2)]
    flags = [_flags_buf(eng, m + k) for _ in range(2)]
    eng.sync()
    for rep in range(4):
        for s in range(2):
            f = L.fhe_baseconv_exact_checked if (rep + s) % 2 == 0 else L.fhe_baseconv_fast_checked
            assert f(eng._h, d_out[s].ptr, d_in[s].ptr, bc._h, N, flags[s].ptr, C.c_void_p(streams[s].cuda_stream)) == 0
    for s in streams:
        s.synchronize()
    # the last repetition: stream 0 ran the fast form, stream 1 the exact one
    assert not _read_flags(flags[0], k).any() and not _read_flags(flags[1], m + k).any()
    assert (d_out[0].download().reshape(k, N) == O.bconv_fast(xs[0], mi, mo).T).all()
    assert (d_out[1].download().reshape(k, N) == O.baseconv_exact(xs[1], mi, mo)).all()
