"""Checked NTT-domain Galois permutation on the GPU: clean calls return fhe_automorphism_ntt's words with every flag zero from a
garbage-filled buffer and leave the source alone; one armed bit flip of a gathered word or of a source index raises exactly its
unit's flag, changes that output word, and leaves the next call clean; bad arguments and hooks are error statuses; the checked
key preparation returns the unchecked one's words."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID = 1
WORD, INDEX = 0, 1


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


@pytest.fixture(scope="module")
def tables(F, eng):
    """per log_n: one table set of 7 limbs (the permutation reads only log_n from it) and 7 rows of arbitrary 64-bit words"""
    out = {}
    for logn in (5, 8, 10, 13):
        N = 1 << logn
        t = eng.tables(logn, F.create_moduli(N, [50] * 7))
        src = np.random.default_rng(logn).integers(0, 1 << 64, (7, N), dtype=np.uint64)
        src[0, :3] = [0, (1 << 32) - 1, (1 << 64) - 1]
        out[logn] = (t, src)
    return out


@pytest.mark.parametrize("logn", [5, 8, 10, 13])
def test_clean_calls_return_the_unchecked_words_and_no_flag(F, eng, tables, logn):
    t, src = tables[logn]
    N = 1 << logn
    for units in (1, 3, 7):
        d = eng.upload(src[:units])
        for k in (1, 3, 5, 125, 2 * N - 1):
            dst, flags = F.automorphism_checked(eng, t, d, k, limbs=units)
            want = F.automorphism(eng, t, d, k, limbs=units, ntt_domain=True)
            assert (dst.download() == want.download()).all(), (units, k)
            assert flags.shape == (units,) and not flags.any(), (units, k, flags.tolist())
        assert (d.download() == src[:units]).all()
    eng.check()


@pytest.mark.parametrize("logn", [5, 8, 10, 13])
def test_one_flip_raises_exactly_its_unit(F, eng, tables, logn):
    from fhe_reliability_gpu_amd._lib import check, lib
    t, src = tables[logn]
    N = 1 << logn
    units, k = 7, 5
    d = eng.upload(src)
    clean, flags = F.automorphism_checked(eng, t, d, k)
    assert not flags.any()
    want = clean.download()
    cases = [(WORD, b) for b in (0, 31, 32, 60, 63)] + [(INDEX, b) for b in (0, logn - 1)]
    n = 0
    for i, (point, bit) in enumerate(cases):
        unit, coeff = (0, 3, 6, 2, 5, 1, 6)[i], (0, N - 1, N // 2 + 3, 1, N - 2, 7, N - 1)[i]
        check(lib.fhe_ctx_inject_fault_galois(eng._h, point, unit, coeff, bit))
        dst, flags = F.automorphism_checked(eng, t, d, k)
        assert np.flatnonzero(flags).tolist() == [unit] and flags[unit] == 1, (point, bit, flags.tolist())
        got = dst.download()
        assert np.argwhere(got != want).tolist() == [[unit, coeff]], (point, bit)
        if point == WORD:
            assert int(got[unit, coeff]) == int(want[unit, coeff]) ^ (1 << bit)
        # one shot: the next call is clean again
        dst, flags = F.automorphism_checked(eng, t, d, k)
        assert not flags.any() and (dst.download() == want).all()
        n += 1
    assert n == 7          # no case skipped
    eng.check()


def test_bad_arguments_and_hooks_are_error_statuses(F, eng, tables):
    from fhe_reliability_gpu_amd._lib import check, lib
    logn = 8
    t, src = tables[logn]
    N = 1 << logn
    d, o = eng.upload(src[:3]), eng.alloc(3 * N)
    fl = eng.alloc(2)

    def call(dst, s, k=3, units=3, flags=fl.ptr):
        return lib.fhe_automorphism_ntt_checked(eng._h, dst, s, logn, k, units, flags, None)

    assert call(o.ptr, d.ptr) == 0
    assert call(o.ptr, d.ptr, k=4) == INVALID                 # even element
    assert call(d.ptr, d.ptr) == INVALID                      # in place
    assert call(None, d.ptr) == INVALID and call(o.ptr, None) == INVALID and call(o.ptr, d.ptr, flags=None) == INVALID
    assert lib.fhe_automorphism_ntt_checked(None, o.ptr, d.ptr, logn, 3, 3, fl.ptr, None) == INVALID
    assert call(o.ptr, d.ptr, units=0) == 0                   # nothing to do
    # hooks outside the call: refused, nothing launched, used up
    for point, unit, coeff, bit in ((WORD, 3, 0, 0), (WORD, 0, N, 0), (INDEX, 0, 0, logn), (INDEX, 2, 5, 63)):
        check(lib.fhe_ctx_inject_fault_galois(eng._h, point, unit, coeff, bit))
        assert call(o.ptr, d.ptr) == INVALID, (point, unit, coeff, bit)
        dst, flags = F.automorphism_checked(eng, t, d, 3, limbs=3)
        assert not flags.any()
    # hooks that do not exist at all
    assert lib.fhe_ctx_inject_fault_galois(eng._h, 2, 0, 0, 0) == INVALID
    assert lib.fhe_ctx_inject_fault_galois(eng._h, WORD, -1, 0, 0) == INVALID
    assert lib.fhe_ctx_inject_fault_galois(eng._h, WORD, 0, -1, 0) == INVALID
    assert lib.fhe_ctx_inject_fault_galois(eng._h, WORD, 0, 0, 64) == INVALID
    # clearing an armed hook
    check(lib.fhe_ctx_inject_fault_galois(eng._h, WORD, 0, 0, 5))
    check(lib.fhe_ctx_inject_fault_galois(eng._h, -1, 0, 0, 0))
    assert not F.automorphism_checked(eng, t, d, 3, limbs=3)[1].any()
    eng.check()


def test_checked_key_preparation_returns_the_unchecked_words(F, eng):
    logn, L, K, dnum = 10, 4, 2, 2
    N = 1 << logn
    qs = F.create_moduli(N, [50] * L + [61] * K)
    t = eng.tables(logn, qs)
    ks = F.KeySwitch(eng, t, L, K, dnum)
    rng = np.random.default_rng(4)
    key = eng.upload(np.stack([np.stack([np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs]) for _ in range(2)]) for _ in range(dnum)]))
    for k in (3, 25, 2 * N - 1):
        got, flags = ks.prepare_galois_key_checked(key, k)
        assert flags.shape == (dnum, 2, L + K) and not flags.any()
        assert (got.download() == ks.prepare_galois_key(key, k).download()).all(), k
    eng.check()
