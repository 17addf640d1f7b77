"""Residue-checked element-wise products on the device (pointwise_checked.hip): fhe_modmul_checked / _acc_checked and
fhe_tensor_product_checked give the unchecked calls' words bit for bit with every flag clear on clean runs, flag exactly
the unit whose word a hook fault changed, and raise only bit 4 on non-canonical operands."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RESIDUE, RANGE, OPERAND = 1, 2, 4
ERR_INVALID, ERR_UNSUPPORTED = 1, 3
GARBAGE = 0xA5A5A5A5DEADBEEF


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


def _rand(rng, qs, polys, N):
    return np.stack([np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs]) for _ in range(polys)])


def _flags_buf(eng, n):
    """a flags buffer pre-filled with garbage: the call must clear it"""
    return eng.upload(np.full((n + 1) // 2, GARBAGE, dtype=np.uint64))


def _read_flags(buf, n):
    return buf.download().view(np.uint32)[:n].copy()


def _ref_modmul(a, b, o, qs, acc):
    """Python-integer reference, [polys][limbs][N]"""
    out = np.empty(a.shape, dtype=np.uint64)
    for l, q in enumerate(qs):
        x = a[:, l].astype(object) * b[:, l].astype(object)
        if acc:
            x = x + o[:, l].astype(object)
        out[:, l] = (x % q).astype(np.uint64)
    return out


def _modmul_checked(eng, L, t, c, a, b, polys, limbs, start, acc, stream=None):
    flags = _flags_buf(eng, polys * limbs)
    f = L.fhe_modmul_acc_checked if acc else L.fhe_modmul_checked
    rc = f(eng._h, c.ptr, a.ptr, b.ptr, t._h, polys, limbs, start, flags.ptr, stream)
    return rc, flags


# (logn, prime sizes): 30-bit primes only up to N = 2^14, as in test_gpu_parity.py; "mixed" tables hold both arithmetic paths
CLEAN = [(1, [30, 30, 30]), (1, [50, 50, 50]), (1, [61, 61, 61]), (1, [50, 61, 30]),
         (10, [30, 30, 30]), (10, [50, 50, 50]), (10, [61, 61, 61]), (10, [61, 30, 50]),
         (16, [50, 50, 50]), (16, [61, 61, 61]), (16, [50, 61, 50]),
         (17, [50, 50, 50]), (17, [61, 61, 61]), (17, [61, 50, 61])]


@pytest.mark.parametrize("logn,bits", CLEAN)
@pytest.mark.parametrize("acc", [False, True])
def test_modmul_checked_clean_matches_unchecked_and_python(F, eng, L, logn, bits, acc):
    from fhe_reliability_gpu_amd._lib import check
    N = 1 << logn
    qs = F.create_moduli(N, bits)
    t = eng.tables(logn, qs)
    rng = np.random.default_rng(logn * 7 + len(set(bits)) + acc)
    start, limbs, polys = 1, 2, 3
    w = qs[start:start + limbs]
    a, b, o = (_rand(rng, w, polys, N) for _ in range(3))
    a[0, 0, 0], b[0, 0, 0] = 0, w[0] - 1                     # edge words
    a[-1, -1, -1], b[-1, -1, -1] = w[-1] - 1, w[-1] - 1
    da, db, dc = eng.upload(a), eng.upload(b), eng.upload(o)
    rc, flags = _modmul_checked(eng, L, t, dc, da, db, polys, limbs, start, acc)
    assert rc == 0
    got = dc.download().reshape(a.shape)
    assert not _read_flags(flags, polys * limbs).any()
    ref = eng.upload(o)
    check((L.fhe_modmul_acc if acc else L.fhe_modmul)(eng._h, ref.ptr, da.ptr, db.ptr, t._h, polys, limbs, start, None))
    assert (got == ref.download().reshape(a.shape)).all()
    assert (got == _ref_modmul(a, b, o, w, acc)).all()


@pytest.mark.parametrize("alias", ["a", "b"])
@pytest.mark.parametrize("acc", [False, True])
def test_modmul_checked_in_place(F, eng, L, alias, acc):
    logn, N = 12, 1 << 12
    qs = F.create_moduli(N, [50, 61, 61, 50])
    t = eng.tables(logn, qs)
    rng = np.random.default_rng(3 + acc)
    start, limbs, polys = 2, 2, 4
    w = qs[start:start + limbs]
    a, b = _rand(rng, w, polys, N), _rand(rng, w, polys, N)
    da, db = eng.upload(a), eng.upload(b)
    dc = da if alias == "a" else db
    old = a if alias == "a" else b
    rc, flags = _modmul_checked(eng, L, t, dc, da, db, polys, limbs, start, acc)
    assert rc == 0
    assert not _read_flags(flags, polys * limbs).any()
    assert (dc.download().reshape(a.shape) == _ref_modmul(a, b, old, w, acc)).all()


def test_modmul_checked_wrapper(F, eng):
    logn, N = 10, 1 << 10
    qs = F.create_moduli(N, [50, 61])
    t = eng.tables(logn, qs)
    rng = np.random.default_rng(11)
    a, b = _rand(rng, qs, 2, N), _rand(rng, qs, 2, N)
    da, db, dc = eng.upload(a), eng.upload(b), eng.alloc(a.size)
    flags = t.modmul_checked(dc, da, db, n_poly=2)
    assert flags.dtype == np.uint32 and flags.shape == (4,) and not flags.any()
    assert (dc.download().reshape(a.shape) == _ref_modmul(a, b, None, qs, False)).all()
    flags = t.modmul_checked(dc, da, db, n_poly=2, acc=True)
    assert not flags.any()
    assert (dc.download().reshape(a.shape) == _ref_modmul(a, b, _ref_modmul(a, b, None, qs, False), qs, True)).all()


@pytest.mark.parametrize("acc", [False, True])
def test_modmul_checked_noncanonical_word_raises_bit_4_on_its_unit_only(F, eng, L, acc):
    from fhe_reliability_gpu_amd._lib import check
    logn, N = 13, 1 << 13
    qs = F.create_moduli(N, [50, 61, 50])
    t = eng.tables(logn, qs)
    rng = np.random.default_rng(21 + acc)
    limbs, polys = 3, 2
    a, b, o = (_rand(rng, qs, polys, N) for _ in range(3))
    a[1, 2, 77] = np.uint64(2**64 - 5)                     # unit 1 * 3 + 2 = 5
    if acc:
        o[0, 1, 5] = np.uint64(qs[1])                       # the old word, exactly q: unit 1
    da, db, dc = eng.upload(a), eng.upload(b), eng.upload(o)
    rc, flags = _modmul_checked(eng, L, t, dc, da, db, polys, limbs, 0, acc)
    assert rc == 0
    f = _read_flags(flags, polys * limbs)
    want = np.zeros(polys * limbs, dtype=np.uint32)
    want[5] = OPERAND
    if acc:
        want[1] = OPERAND
    assert (f == want).all()
    ref = eng.upload(o)
    check((L.fhe_modmul_acc if acc else L.fhe_modmul)(eng._h, ref.ptr, da.ptr, db.ptr, t._h, polys, limbs, 0, None))
    assert (dc.download() == ref.download()).all()


# ---- tensor product ----------------------------------------------------------------------------------------------------
def _tensor_checked(eng, L, t, limbs, start, ops, fl=None):
    d = [eng.alloc(limbs * t.N) for _ in range(3)]
    flags = fl if fl is not None else _flags_buf(eng, 3 * limbs)
    rc = L.fhe_tensor_product_checked(eng._h, d[0].ptr, d[1].ptr, d[2].ptr, ops[0].ptr, ops[1].ptr, ops[2].ptr, ops[3].ptr, t._h, limbs,
                                      start, flags.ptr, None)
    return rc, [x.download().reshape(limbs, t.N) for x in d], flags


def _tensor_plain(eng, L, t, limbs, start, ops):
    from fhe_reliability_gpu_amd._lib import check
    d = [eng.alloc(limbs * t.N) for _ in range(3)]
    check(L.fhe_tensor_product(eng._h, d[0].ptr, d[1].ptr, d[2].ptr, ops[0].ptr, ops[1].ptr, ops[2].ptr, ops[3].ptr, t._h, limbs, start, None))
    return [x.download().reshape(limbs, t.N) for x in d]


def test_tensor_checked_config4_shape(F, eng, L):
    # BASELINE config 4 (N = 2^17, L = 32): both arithmetic paths, every word against fhe_tensor_product
    logn, N, limbs = 17, 1 << 17, 32
    qs = F.create_moduli(N, [50 if i % 4 else 61 for i in range(limbs)])
    t = eng.tables(logn, qs)
    assert set(t.paths) == {0, 1}
    rng = np.random.default_rng(17)
    host = [np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs]) for _ in range(4)]
    ops = [eng.upload(h) for h in host]
    rc, got, flags = _tensor_checked(eng, L, t, limbs, 0, ops)
    assert rc == 0
    assert not _read_flags(flags, 3 * limbs).any()
    want = _tensor_plain(eng, L, t, limbs, 0, ops)
    for k in range(3):
        assert (got[k] == want[k]).all()
    # and a Python-integer spot check on a sample of columns of every limb
    a0, a1, b0, b1 = host
    cols = rng.integers(0, N, 64)
    for l, q in enumerate(qs):
        for i in cols:
            x0, x1, y0, y1 = int(a0[l, i]), int(a1[l, i]), int(b0[l, i]), int(b1[l, i])
            assert (int(got[0][l, i]), int(got[1][l, i]), int(got[2][l, i])) == (x0 * y0 % q, (x0 * y1 + x1 * y0) % q, x1 * y1 % q)


@pytest.mark.parametrize("logn", [1, 10])
def test_tensor_checked_limb_window(F, eng, L, logn):
    N = 1 << logn
    qs = F.create_moduli(N, [30, 50, 61, 50, 61])
    t = eng.tables(logn, qs)
    rng = np.random.default_rng(logn)
    start, limbs = 1, 3
    ops = [eng.upload(np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs[start:start + limbs]])) for _ in range(4)]
    rc, got, flags = _tensor_checked(eng, L, t, limbs, start, ops)
    assert rc == 0 and not _read_flags(flags, 3 * limbs).any()
    want = _tensor_plain(eng, L, t, limbs, start, ops)
    assert all((g == w).all() for g, w in zip(got, want))


def test_tensor_checked_wrapper(F, eng):
    logn, N = 12, 1 << 12
    Lc, K, dnum = 3, 1, 3
    qs = F.create_moduli(N, [50, 61, 50, 61])
    t = eng.tables(logn, qs)
    ks = F.KeySwitch(eng, t, Lc, K, dnum)
    rng = np.random.default_rng(5)
    host = [np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs[:Lc]]) for _ in range(4)]
    ops = [eng.upload(h) for h in host]
    d0, d1, d2, flags = ks.tensor_checked(*ops)
    assert flags.shape == (Lc, 3) and not flags.any()
    w0, w1, w2 = ks.tensor(*ops)
    for g, w in ((d0, w0), (d1, w1), (d2, w2)):
        assert (g.download() == w.download()).all()


def test_tensor_checked_noncanonical_word(F, eng, L):
    logn, N = 11, 1 << 11
    qs = F.create_moduli(N, [50, 61])
    t = eng.tables(logn, qs)
    rng = np.random.default_rng(9)
    host = [np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs]) for _ in range(4)]
    host[0][1, 300] = np.uint64(2**64 - 1)                 # a0 of limb 1: d0 and d1 of limb 1
    host[3][0, 7] = np.uint64(qs[0] + 3)                   # b1 of limb 0: d1 and d2 of limb 0
    ops = [eng.upload(h) for h in host]
    rc, got, flags = _tensor_checked(eng, L, t, 2, 0, ops)
    assert rc == 0
    assert (_read_flags(flags, 6).reshape(2, 3) == np.array([[0, OPERAND, OPERAND], [OPERAND, OPERAND, 0]], dtype=np.uint32)).all()
    want = _tensor_plain(eng, L, t, 2, 0, ops)
    assert all((g == w).all() for g, w in zip(got, want))


# ---- the test hook -----------------------------------------------------------------------------------------------------
def _arm(L, point, idx, bit):
    from fhe_reliability_gpu_amd._lib import check
    from fhe_reliability_gpu_amd import default_engine
    check(L.fhe_ctx_inject_fault_pointwise(default_engine()._h, point, idx, bit))


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("bits", [[50, 61, 50], [61, 30, 61]])
def test_modmul_hook_flags_exactly_the_changed_unit(F, eng, L, acc, bits):
    logn, N = 10, 1 << 10
    qs = F.create_moduli(N, bits)
    t = eng.tables(logn, qs)
    rng = np.random.default_rng(31 + acc)
    limbs, polys = 3, 2
    a, b, o = (_rand(rng, qs, polys, N) for _ in range(3))
    da, db = eng.upload(a), eng.upload(b)
    dc = eng.upload(o)
    rc, flags = _modmul_checked(eng, L, t, dc, da, db, polys, limbs, 0, acc)
    assert rc == 0 and not _read_flags(flags, polys * limbs).any()
    clean = dc.download().ravel()
    points = [0, 1, 2, 3] if acc else [0, 1, 2]
    seen_changed = 0
    for point in points:
        for unit, bit in ((0, 0), (1, 5), (3, 31), (4, 47), (5, 63), (2, 1)):
            idx = unit * N + (bit * 37) % N
            dc = eng.upload(o)
            _arm(L, point, idx, bit)
            rc, flags = _modmul_checked(eng, L, t, dc, da, db, polys, limbs, 0, acc)
            assert rc == 0
            got = dc.download().ravel()
            f = _read_flags(flags, polys * limbs)
            diff = np.nonzero(got != clean)[0]
            assert set(diff.tolist()) <= {idx}, f"point {point}: a word other than the target changed"
            changed = diff.size > 0
            seen_changed += changed
            others = np.delete(f, unit)
            assert not others.any(), f"point {point} bit {bit}: a unit other than {unit} was flagged"
            assert bool(f[unit]) == changed, f"point {point} bit {bit}: word changed {changed}, flags {f[unit]}"
            assert not (f[unit] & OPERAND)
    assert seen_changed >= len(points) * 4
    # the hook is one-shot: the next call is clean
    dc = eng.upload(o)
    rc, flags = _modmul_checked(eng, L, t, dc, da, db, polys, limbs, 0, acc)
    assert rc == 0 and not _read_flags(flags, polys * limbs).any() and (dc.download().ravel() == clean).all()


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("elem", ["last of the last unit", "a lane's second word"])
def test_modmul_hook_addresses_unit_and_coefficient_at_the_smallest_shape(F, eng, L, acc, elem):
    # N = 2: one lane holds a whole unit, so the hook's element index has to split into (unit, coefficient) exactly; the window
    # starts at limb 1 of the tables, so a unit is not a table limb either
    logn, N = 1, 2
    qs = F.create_moduli(N, [50, 61, 50])
    t = eng.tables(logn, qs)
    start, limbs, polys = 1, 2, 2
    w = qs[start:start + limbs]
    rng = np.random.default_rng(41 + acc)
    a, b, o = (_rand(rng, w, polys, N) for _ in range(3))
    da, db = eng.upload(a), eng.upload(b)
    clean = _ref_modmul(a, b, o, w, acc).ravel()
    idx = polys * limbs * N - 1 if elem == "last of the last unit" else 1
    unit = idx // N
    dc = eng.upload(o)
    _arm(L, 2, idx, 0)                                       # the word itself, lowest bit: it always changes
    rc, flags = _modmul_checked(eng, L, t, dc, da, db, polys, limbs, start, acc)
    assert rc == 0
    got = dc.download().ravel()
    assert np.nonzero(got != clean)[0].tolist() == [idx] and int(got[idx]) == int(clean[idx]) ^ 1
    f = _read_flags(flags, polys * limbs)
    assert f[unit] and not (f[unit] & OPERAND) and not np.delete(f, unit).any()


@pytest.mark.parametrize("bits", [[50, 61], [61, 50]])
def test_tensor_hook_addresses_limb_and_coefficient_at_the_smallest_shape(F, eng, L, bits):
    logn, N, limbs = 1, 2, 2
    qs = F.create_moduli(N, bits)
    t = eng.tables(logn, qs)
    rng = np.random.default_rng(sum(bits) + bits[0])
    ops = [eng.upload(np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs])) for _ in range(4)]
    rc, clean, flags = _tensor_checked(eng, L, t, limbs, 0, ops)
    assert rc == 0 and not _read_flags(flags, 3 * limbs).any()
    idx = limbs * N - 1                                      # the last element: limb 1, coefficient 1
    _arm(L, 2, idx, 0)
    rc, got, flags = _tensor_checked(eng, L, t, limbs, 0, ops)
    assert rc == 0
    assert (got[0] == clean[0]).all() and (got[2] == clean[2]).all()
    assert np.nonzero(got[1].ravel() != clean[1].ravel())[0].tolist() == [idx] and int(got[1][1, 1]) == int(clean[1][1, 1]) ^ 1
    f = _read_flags(flags, 3 * limbs).reshape(limbs, 3)
    assert f[1, 1] and not np.delete(f.ravel(), 3 * 1 + 1).any()


def test_modmul_hook_point_3_needs_a_running_sum(F, eng, L):
    logn, N = 8, 1 << 8
    qs = F.create_moduli(N, [50])
    t = eng.tables(logn, qs)
    rng = np.random.default_rng(2)
    a, b = _rand(rng, qs, 1, N), _rand(rng, qs, 1, N)
    da, db = eng.upload(a), eng.upload(b)
    sentinel = np.full(a.shape, 7, dtype=np.uint64)
    dc = eng.upload(sentinel)
    _arm(L, 3, 5, 2)
    rc, _ = _modmul_checked(eng, L, t, dc, da, db, 1, 1, 0, False)
    assert rc == ERR_UNSUPPORTED
    assert (dc.download() == sentinel).all()                # nothing was launched
    rc, flags = _modmul_checked(eng, L, t, dc, da, db, 1, 1, 0, False)     # the hook was used up
    assert rc == 0 and not _read_flags(flags, 1).any()
    assert (dc.download().reshape(a.shape) == _ref_modmul(a, b, None, qs, False)).all()


@pytest.mark.parametrize("bits", [[50, 50, 50], [61, 61, 61], [50, 61, 50]])
def test_tensor_hook_flags_exactly_the_changed_d1_word(F, eng, L, bits):
    logn, N = 11, 1 << 11
    qs = F.create_moduli(N, bits)
    t = eng.tables(logn, qs)
    rng = np.random.default_rng(sum(bits))
    limbs = 3
    ops = [eng.upload(np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs])) for _ in range(4)]
    rc, clean, flags = _tensor_checked(eng, L, t, limbs, 0, ops)
    assert rc == 0 and not _read_flags(flags, 3 * limbs).any()
    seen_changed = 0
    for point in (0, 1, 2, 3):
        for l, bit in ((0, 0), (1, 13), (2, 40), (0, 52), (1, 62), (2, 1)):
            idx = l * N + (bit * 53 + 1) % N
            _arm(L, point, idx, bit)
            rc, got, flags = _tensor_checked(eng, L, t, limbs, 0, ops)
            assert rc == 0
            assert (got[0] == clean[0]).all() and (got[2] == clean[2]).all()
            diff = np.nonzero(got[1].ravel() != clean[1].ravel())[0]
            assert set(diff.tolist()) <= {idx}
            changed = diff.size > 0
            seen_changed += changed
            f = _read_flags(flags, 3 * limbs)
            others = np.delete(f, 3 * l + 1)
            assert not others.any(), f"point {point} bit {bit}: another unit flagged"
            assert bool(f[3 * l + 1]) == changed, f"point {point} limb {l} bit {bit}: word changed {changed}, flags {f[3 * l + 1]}"
    assert seen_changed >= 12
    rc, got, flags = _tensor_checked(eng, L, t, limbs, 0, ops)
    assert rc == 0 and not _read_flags(flags, 3 * limbs).any() and all((g == c).all() for g, c in zip(got, clean))


def test_bad_arguments_return_statuses(F, eng, L):
    logn, N = 6, 1 << 6
    qs = F.create_moduli(N, [50, 61])
    t = eng.tables(logn, qs)
    x = eng.upload(_rand(np.random.default_rng(0), qs, 1, N))
    fl = _flags_buf(eng, 8)
    for f in (L.fhe_modmul_checked, L.fhe_modmul_acc_checked):
        assert f(eng._h, x.ptr, x.ptr, x.ptr, t._h, 1, 2, 0, None, None) == ERR_INVALID        # null flags
        assert f(eng._h, x.ptr, x.ptr, x.ptr, t._h, 1, 2, 1, fl.ptr, None) == ERR_INVALID      # window past the tables
        assert f(eng._h, None, x.ptr, x.ptr, t._h, 1, 2, 0, fl.ptr, None) == ERR_INVALID
        assert f(eng._h, x.ptr, x.ptr, x.ptr, None, 1, 2, 0, fl.ptr, None) == ERR_INVALID
    tp = L.fhe_tensor_product_checked
    assert tp(eng._h, x.ptr, x.ptr, x.ptr, x.ptr, x.ptr, x.ptr, x.ptr, t._h, 2, 0, None, None) == ERR_INVALID
    assert tp(eng._h, x.ptr, x.ptr, x.ptr, x.ptr, x.ptr, x.ptr, x.ptr, t._h, 2, 1, fl.ptr, None) == ERR_INVALID
    assert tp(eng._h, x.ptr, None, x.ptr, x.ptr, x.ptr, x.ptr, x.ptr, t._h, 2, 0, fl.ptr, None) == ERR_INVALID
    assert L.fhe_ctx_inject_fault_pointwise(eng._h, 4, 0, 0) == ERR_INVALID
    assert L.fhe_ctx_inject_fault_pointwise(eng._h, 0, 0, 64) == ERR_INVALID
    assert L.fhe_ctx_inject_fault_pointwise(eng._h, 0, -1, 0) == ERR_INVALID
    assert L.fhe_ctx_inject_fault_pointwise(None, 0, 0, 0) == ERR_INVALID
    # a fault outside the call's window is refused (and used up)
    assert L.fhe_ctx_inject_fault_pointwise(eng._h, 2, 2 * N, 0) == 0
    assert L.fhe_modmul_checked(eng._h, x.ptr, x.ptr, x.ptr, t._h, 1, 2, 0, fl.ptr, None) == ERR_INVALID
    assert L.fhe_ctx_inject_fault_pointwise(eng._h, 1, 0, 3) == 0
    assert L.fhe_ctx_inject_fault_pointwise(eng._h, -1, 0, 0) == 0                             # cleared
    y = eng.alloc(2 * N)
    assert L.fhe_modmul_checked(eng._h, y.ptr, x.ptr, x.ptr, t._h, 1, 2, 0, fl.ptr, None) == 0
    assert not _read_flags(fl, 2).any()
