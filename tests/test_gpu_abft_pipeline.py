"""On-device ABFT detector beyond the forward transform: the checked inverse NTT and the checked negacyclic product
(the protected chain transform -> element-wise product -> transform of rfhe_framewk/src/four_step_ntt_protected.py:219-282),
clean runs against the oracle and the unchecked calls, and in-flight bit flips at every hook point."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


@pytest.fixture(scope="module")
def O():
    from oracle import cport
    return cport


@pytest.fixture()
def small_chunks(eng):
    # force the sub-batched path (as tests/test_gpu_subbatch.py does), restore the defaults afterwards
    eng.set_option("ntt_chunk_mib", 1)
    eng.set_option("ntt_chunk_floor_mib", 0)
    yield
    eng.set_option("ntt_chunk_mib", 96)
    eng.set_option("ntt_chunk_floor_mib", 192)


def _rand(rng, qs, polys, N):
    return np.stack([np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs]) for _ in range(polys)])


@pytest.mark.parametrize("logn", [1, 4, 5, 8, 12, 13, 15, 16, 17])
def test_inverse_checked_every_plan_shape(F, eng, O, logn):
    N = 1 << logn
    qs = F.create_moduli(N, [50, 61, 61, 50])
    t = eng.tables(logn, qs)
    ab = F.Abft(eng, t)
    rng = np.random.default_rng(100 + logn)
    start, limbs, polys = 1, 3, 2
    data = _rand(rng, qs[start:start + limbs], polys, N)
    data[1, 0, N // 2] = np.uint64(2**64 - 5)               # an out-of-range word: reduced modulo its prime on both sides
    d = eng.upload(data)
    flags = ab.inverse_checked(d, n_poly=polys, limbs=limbs, start=start)
    assert not flags.any()
    got = d.download()
    ref = eng.upload(data)
    t.inverse(ref, limbs=limbs, start=start, n_poly=polys)
    assert (got == ref.download()).all()
    for p in range(polys):
        for l in range(limbs):
            q = qs[start + l]
            assert (got[p, l] == O.nwt_inverse(data[p, l] % np.uint64(q), q, O.root_powers(q, logn))).all()


@pytest.mark.parametrize("logn", [5, 13, 16])
def test_forward_then_inverse_checked_round_trip(F, eng, logn):
    N = 1 << logn
    qs = F.create_moduli(N, [50, 61])
    t = eng.tables(logn, qs)
    ab = F.Abft(eng, t)
    data = _rand(np.random.default_rng(logn), qs, 3, N)
    d = eng.upload(data)
    assert not ab.forward_checked(d, n_poly=3).any()
    assert not ab.inverse_checked(d, n_poly=3).any()
    assert (d.download() == data).all()


@pytest.mark.parametrize("logn,bits,limbs,polys", [(14, 50, 3, 4), (14, 61, 3, 4), (16, 50, 2, 3)])
def test_inverse_checked_flags_only_the_unit_hit_in_flight(F, eng, logn, bits, limbs, polys):
    from fhe_reliability_gpu_amd._lib import check, lib
    N = 1 << logn
    qs = F.create_moduli(N, [bits] * limbs)
    t = eng.tables(logn, qs)
    ab = F.Abft(eng, t)
    data = _rand(np.random.default_rng(logn + bits), qs, polys, N)
    d = eng.upload(data)
    assert not ab.inverse_checked(d, n_poly=polys).any()
    clean = d.download().reshape(polys * limbs, N)
    for unit, word, bit in ((5 % (polys * limbs), 1234, 7), (0, 0, 30), (polys * limbs - 1, N - 1, 3)):
        d = eng.upload(data)
        check(lib.fhe_ctx_inject_fault(eng._h, unit * N + word, bit))
        flags = ab.inverse_checked(d, n_poly=polys)
        assert flags.tolist() == [1 if u == unit else 0 for u in range(polys * limbs)], (unit, flags)
        bad = (d.download().reshape(polys * limbs, N) != clean).any(axis=1)
        assert bad.tolist() == [u == unit for u in range(polys * limbs)]
    # a fault already present in the input is not a transform fault
    faulty = data.copy()
    faulty[1, limbs - 1, 77] ^= np.uint64(1 << 5)
    d = eng.upload(faulty)
    assert not ab.inverse_checked(d, n_poly=polys).any()


def test_inverse_checked_sub_batches(F, eng, small_chunks):
    from fhe_reliability_gpu_amd._lib import check, lib
    logn, N, limbs, polys = 14, 1 << 14, 2, 24
    qs = F.create_moduli(N, [50, 61])
    t = eng.tables(logn, qs)
    ab = F.Abft(eng, t)
    data = _rand(np.random.default_rng(5), qs, polys, N)
    d = eng.upload(data)
    assert not ab.inverse_checked(d, n_poly=polys).any()
    ref = eng.upload(data)
    t.inverse(ref, n_poly=polys)
    assert (d.download() == ref.download()).all()
    unit = 17
    d = eng.upload(data)
    check(lib.fhe_ctx_inject_fault(eng._h, unit * N + 999, 11))
    flags = ab.inverse_checked(d, n_poly=polys)
    assert flags.tolist() == [1 if u == unit else 0 for u in range(polys * limbs)]


def _polymul_ref(O, a, b, qs, N):
    out = np.empty_like(a)
    for p in range(a.shape[0]):
        for l, q in enumerate(qs):
            out[p, l] = O.polymul_ntt(a[p, l], b[p, l], O.min_primitive_root(q, 2 * N), q)
    return out


@pytest.mark.parametrize("logn", [2, 4, 5, 8, 12, 13, 14, 16, 17])
def test_polymul_checked_clean(F, eng, O, logn):
    N = 1 << logn
    qs = F.create_moduli(N, [50, 61, 50])
    t = eng.tables(logn, qs)
    ab = F.Abft(eng, t)
    start, limbs, polys = 1, 2, 2
    rng = np.random.default_rng(200 + logn)
    a = _rand(rng, qs[start:], polys, N)
    b = _rand(rng, qs[start:], polys, N)
    want = _polymul_ref(O, a, b, qs[start:], N)
    # plain call, c separate
    da, db, dc = eng.upload(a), eng.upload(b), eng.upload(np.zeros_like(a))
    flags = ab.polymul_checked(dc, da, db, n_poly=polys, limbs=limbs, start=start)
    assert flags.shape == (polys * limbs, 3) and not flags.any()
    got = dc.download()
    assert (got == want).all()
    ua, ub, uc = eng.upload(a), eng.upload(b), eng.upload(np.zeros_like(a))
    t.polymul(uc, ua, ub, limbs=limbs, start=start, n_poly=polys)
    assert (got == uc.download()).all()
    # c aliasing a
    da, db = eng.upload(a), eng.upload(b)
    assert not ab.polymul_checked(da, da, db, n_poly=polys, limbs=limbs, start=start).any()
    assert (da.download() == want).all()
    # squaring: a is b
    da = eng.upload(a)
    assert not ab.polymul_checked(da, da, da, n_poly=polys, limbs=limbs, start=start).any()
    assert (da.download() == _polymul_ref(O, a, a, qs[start:], N)).all()


def test_polymul_checked_sub_batches(F, eng, O, small_chunks):
    logn, N, limbs, polys = 14, 1 << 14, 2, 12
    qs = F.create_moduli(N, [50, 61])
    t = eng.tables(logn, qs)
    ab = F.Abft(eng, t)
    rng = np.random.default_rng(9)
    a, b = _rand(rng, qs, polys, N), _rand(rng, qs, polys, N)
    da, db, dc = eng.upload(a), eng.upload(b), eng.upload(np.zeros_like(a))
    assert not ab.polymul_checked(dc, da, db, n_poly=polys).any()
    assert (dc.download() == _polymul_ref(O, a, b, qs, N)).all()


@pytest.mark.parametrize("logn,point", [(14, 0), (14, 1), (14, 2), (14, 3), (16, 0), (16, 1), (16, 2), (16, 3), (10, 2)])
def test_polymul_checked_hook_points(F, eng, logn, point):
    from fhe_reliability_gpu_amd._lib import check, lib
    N = 1 << logn
    limbs, polys = 2, 3
    qs = F.create_moduli(N, [50, 61])
    t = eng.tables(logn, qs)
    ab = F.Abft(eng, t)
    rng = np.random.default_rng(300 + logn + point)
    a, b = _rand(rng, qs, polys, N), _rand(rng, qs, polys, N)
    da, db, dc = eng.upload(a), eng.upload(b), eng.upload(np.zeros_like(a))
    assert not ab.polymul_checked(dc, da, db, n_poly=polys).any()
    clean = dc.download().reshape(polys * limbs, N)
    want_k = {0: 0, 1: 1, 2: 2, 3: 2}[point]
    for unit, word, bit in ((1, 77, 21), (polys * limbs - 1, N - 3, 33), (2, N // 2, 9)):
        da, db, dc = eng.upload(a), eng.upload(b), eng.upload(np.zeros_like(a))
        check(lib.fhe_ctx_inject_fault_polymul(eng._h, point, unit * N + word, bit))
        flags = ab.polymul_checked(dc, da, db, n_poly=polys)
        want = np.zeros((polys * limbs, 3), dtype=np.uint32)
        want[unit, want_k] = 1
        assert (flags == want).all(), (point, unit, flags)
        bad = (dc.download().reshape(polys * limbs, N) != clean).any(axis=1)
        assert bad.tolist() == [u == unit for u in range(polys * limbs)]


def test_polymul_checked_hook_misuse(F, eng):
    from fhe_reliability_gpu_amd._lib import FheError, check, lib
    logn, N = 10, 1 << 10
    qs = F.create_moduli(N, [50])
    t = eng.tables(logn, qs)
    ab = F.Abft(eng, t)
    a = _rand(np.random.default_rng(1), qs, 1, N)
    for point in (0, 1, 3):                                   # no launch boundary between the steps at a one-launch size
        da, db, dc = eng.upload(a), eng.upload(a), eng.upload(np.zeros_like(a))
        check(lib.fhe_ctx_inject_fault_polymul(eng._h, point, 5, 3))
        with pytest.raises(FheError):
            ab.polymul_checked(dc, da, db)
        assert (da.download() == a).all()                     # nothing was launched
    assert lib.fhe_ctx_inject_fault_polymul(eng._h, 4, 0, 0) != 0
    assert lib.fhe_ctx_inject_fault_polymul(eng._h, 0, 0, 64) != 0
    check(lib.fhe_ctx_inject_fault_polymul(eng._h, -1, 0, 0))
    da, db, dc = eng.upload(a), eng.upload(a), eng.upload(np.zeros_like(a))
    assert not ab.polymul_checked(dc, da, db).any()           # the hook is one shot: a clean call after a refused one
