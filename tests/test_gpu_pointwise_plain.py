"""The plain pointwise calls fhe_modadd, fhe_modsub and fhe_scalar_affine, called directly and compared with Python-integer results:
limb windows (start_idx, a dense buffer of the window's limbs per polynomial), several polynomials, every aliasing the callers use,
and operands outside [0, q) -- all three calls take any 64-bit word for its residue modulo q."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BITS = [50, 61, 30, 61]
LOGNS = [1, 8, 12]                          # 1: the smallest transform size a table set accepts
SHAPES = [(1, 0, 4), (3, 0, 4), (1, 1, 2), (3, 1, 2)]      # n_poly, start_idx, limbs
ERR_INVALID, ERR_UNSUPPORTED = 1, 3
SENTINEL = 0x5E5E5E5E5E5E5E5E
TOP = 2**64 - 1


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


@pytest.fixture(scope="module")
def tables(F, eng):
    made = {}

    def get(logn):
        if logn not in made:
            made[logn] = eng.tables(logn, F.create_moduli(1 << logn, BITS))
        return made[logn]
    return get


def _edge_pairs(q, r):
    """(a, b): the edge words, and the pairs at which a sum or a difference wraps"""
    singles = [0, 1, q - 1, q, q + 1, TOP]
    return [(q - r, r), (q - 1 - r, r), (r, r), (r, r + 1),             # a + b = q, a + b = q - 1, a - b = 0, a < b by one
            (1, q - 1), (q - 1, q - 1), (0, 0), (0, 1), (q + 1, 1), (q, q), (TOP, TOP), (TOP, 0), (0, TOP), (q + r, r + 1),
            (q - 1, 0), (0, q - 1)] + [(s, singles[(i + 1) % 6]) for i, s in enumerate(singles)]


def _operands(qs, n_poly, N, seed):
    """a, b as [n_poly * limbs + 1][N]: random words (two in three canonical, the third any 64-bit word) with the edge pairs at the
    head of every limb -- as many as N holds, starting at another pair in every row -- and a sentinel row behind the batch"""
    rng = np.random.default_rng(seed)
    limbs = len(qs)
    a, b = (np.empty((n_poly * limbs + 1, N), dtype=np.uint64) for _ in range(2))
    for row in range(n_poly * limbs):
        q = qs[row % limbs]
        for x in (a, b):
            x[row] = rng.integers(0, q, N, dtype=np.uint64)
            x[row, 2::3] = rng.integers(0, TOP, len(x[row, 2::3]), dtype=np.uint64, endpoint=True)
        pairs = _edge_pairs(q, int(rng.integers(1, q - 1)))
        for i in range(min(N, len(pairs))):
            a[row, i], b[row, i] = pairs[(i + row * N) % len(pairs)]
    a[-1] = b[-1] = SENTINEL
    return a, b


def _ints(x):
    return x.astype(object)


def _q_column(qs, n_poly):
    """the modulus of every row of a batch, as Python integers [rows][1]"""
    return np.array([int(q) for q in qs] * n_poly, dtype=object).reshape(-1, 1)


def _run(eng, call, c, a, b):
    """c, a, b: host arrays, or the name of the operand that c (or b) aliases -> the words of c after the call, and of the operands"""
    bufs = {}
    bufs["a"] = eng.upload(a)
    bufs["b"] = bufs["a"] if isinstance(b, str) else eng.upload(b)
    bufs["c"] = bufs[c] if isinstance(c, str) else eng.upload(c)
    assert call(bufs["c"].ptr, bufs["a"].ptr, bufs["b"].ptr) == 0
    eng.sync()
    return {k: v.download().reshape(a.shape) for k, v in bufs.items()}


def _assert_words(got, want, sentinel_row=True):
    if sentinel_row:
        assert (got[-1] == SENTINEL).all(), "the call wrote behind its batch"
        got = got[:-1]
    bad = np.argwhere(got != want.astype(np.uint64))
    assert not len(bad), (bad[:8].tolist(), [hex(int(got[tuple(i)])) for i in bad[:8]])


@pytest.mark.parametrize("op", ["add", "sub"])
@pytest.mark.parametrize("n_poly,start,limbs", SHAPES)
@pytest.mark.parametrize("logn", LOGNS)
def test_modadd_modsub(F, eng, L, tables, op, logn, n_poly, start, limbs):
    t, N = tables(logn), 1 << logn
    qs = t.moduli[start:start + limbs]
    a, b = _operands(qs, n_poly, N, logn * 100 + n_poly * 10 + start)
    f = L.fhe_modadd if op == "add" else L.fhe_modsub
    call = lambda c, x, y: f(eng._h, c, x, y, t._h, n_poly, limbs, start, None)
    q = _q_column(qs, n_poly)
    ra, rb = _ints(a[:-1]) % q, _ints(b[:-1]) % q
    want = (ra + rb) % q if op == "add" else (ra - rb) % q
    want_same = (ra + ra) % q if op == "add" else (ra - ra) % q
    fresh = np.full_like(a, SENTINEL)
    # c separate: the operands stay as they were
    out = _run(eng, call, fresh, a, b)
    _assert_words(out["c"], want)
    assert (out["a"] == a).all() and (out["b"] == b).all()
    # c = a, c = b
    _assert_words(_run(eng, call, "a", a, b)["c"], want)
    _assert_words(_run(eng, call, "b", a, b)["c"], want)
    # a = b, and all three the same buffer
    _assert_words(_run(eng, call, fresh, a, "a")["c"], want_same)
    _assert_words(_run(eng, call, "a", a, "a")["c"], want_same)


def _scalars(qs, kind_shift):
    """one scalar per limb: 0, 1, q - 1, q, q + 5, 2^64 - 1, another kind on every limb and for every shift"""
    return [[0, 1, q - 1, q, q + 5, TOP][(l + kind_shift) % 6] for l, q in enumerate(qs)]


@pytest.mark.parametrize("n_poly,start,limbs", SHAPES)
@pytest.mark.parametrize("logn", LOGNS)
def test_scalar_affine(F, eng, L, tables, logn, n_poly, start, limbs):
    """c = (a mod q) mul + add mod q for ANY 64-bit word a and any 64-bit scalars; both scalar arrays NULL is a mod q."""
    t, N = tables(logn), 1 << logn
    qs = t.moduli[start:start + limbs]
    a, _ = _operands(qs, n_poly, N, logn * 100 + n_poly * 10 + start + 5)
    q = _q_column(qs, n_poly)
    ia = _ints(a[:-1])
    arr = lambda v: None if v is None else (C.c_uint64 * limbs)(*v)
    col = lambda v: np.array([int(s) for s in v] * n_poly, dtype=object).reshape(-1, 1)
    cases = [(None, None)]
    for shift in range(6):
        mul, add = _scalars(qs, shift), _scalars(qs, shift + 2)
        cases += [(mul, None), (None, add), (mul, add)]
    for i, (mul, add) in enumerate(cases):
        call = lambda c, x, _y: L.fhe_scalar_affine(eng._h, c, x, arr(mul), arr(add), t._h, n_poly, limbs, start, None)
        want = (ia * (1 if mul is None else col(mul)) + (0 if add is None else col(add))) % q
        if i % 2:                                   # in place, as every internal caller uses it
            _assert_words(_run(eng, call, "a", a, "a")["c"], want)
        else:
            out = _run(eng, call, np.full_like(a, SENTINEL), a, "a")
            _assert_words(out["c"], want)
            assert (out["a"] == a).all()
    # (separate and in place both ran with both arrays given)
    assert {i % 2 for i, (m_, a_) in enumerate(cases) if m_ and a_} == {0, 1}


def test_scalar_affine_limb_limit(F, eng, L):
    """64 limbs per call are taken, 65 are refused before anything is launched"""
    logn, N = 4, 16
    qs = F.create_moduli(1 << 10, [50] * 60 + [61] * 5)
    t = eng.tables(logn, qs)                     # 65 limbs in the table set: only the call's own limit refuses 65
    rng = np.random.default_rng(64)
    a = np.stack([rng.integers(0, TOP, N, dtype=np.uint64, endpoint=True) for _ in range(65)])
    mul = [int(v) for v in rng.integers(0, TOP, 65, dtype=np.uint64, endpoint=True)]
    add = [int(v) for v in rng.integers(0, TOP, 65, dtype=np.uint64, endpoint=True)]
    d_a, d_c = eng.upload(a), eng.upload(np.full_like(a, SENTINEL))
    arr = lambda v, n: (C.c_uint64 * n)(*v[:n])
    assert L.fhe_scalar_affine(eng._h, d_c.ptr, d_a.ptr, arr(mul, 65), arr(add, 65), t._h, 1, 65, 0, None) == ERR_UNSUPPORTED
    eng.sync()
    assert (d_c.download() == SENTINEL).all()
    assert L.fhe_scalar_affine(eng._h, d_c.ptr, d_a.ptr, arr(mul, 64), arr(add, 64), t._h, 1, 64, 0, None) == 0
    eng.sync()
    got = d_c.download().reshape(65, N)
    q = _q_column(qs[:64], 1)
    want = (_ints(a[:64]) * np.array(mul[:64], dtype=object).reshape(-1, 1) + np.array(add[:64], dtype=object).reshape(-1, 1)) % q
    _assert_words(got, want)                     # (row 64 still holds the sentinel)


def test_statuses(F, eng, L, tables):
    t, N = tables(8), 1 << 8
    a, b = _operands(t.moduli, 1, N, 3)
    d_a, d_b, d_c = eng.upload(a), eng.upload(b), eng.upload(np.full_like(a, SENTINEL))
    for f in (L.fhe_modadd, L.fhe_modsub):
        assert f(None, d_c.ptr, d_a.ptr, d_b.ptr, t._h, 1, 4, 0, None) == ERR_INVALID
        assert f(eng._h, None, d_a.ptr, d_b.ptr, t._h, 1, 4, 0, None) == ERR_INVALID
        assert f(eng._h, d_c.ptr, None, d_b.ptr, t._h, 1, 4, 0, None) == ERR_INVALID
        assert f(eng._h, d_c.ptr, d_a.ptr, None, t._h, 1, 4, 0, None) == ERR_INVALID
        assert f(eng._h, d_c.ptr, d_a.ptr, d_b.ptr, None, 1, 4, 0, None) == ERR_INVALID
        assert f(eng._h, d_c.ptr, d_a.ptr, d_b.ptr, t._h, 1, 4, 1, None) == ERR_INVALID        # the window leaves the table set
    one = (C.c_uint64 * 4)(1, 1, 1, 1)
    f = L.fhe_scalar_affine
    assert f(None, d_c.ptr, d_a.ptr, one, one, t._h, 1, 4, 0, None) == ERR_INVALID
    assert f(eng._h, None, d_a.ptr, one, one, t._h, 1, 4, 0, None) == ERR_INVALID
    assert f(eng._h, d_c.ptr, None, one, one, t._h, 1, 4, 0, None) == ERR_INVALID
    assert f(eng._h, d_c.ptr, d_a.ptr, one, one, None, 1, 4, 0, None) == ERR_INVALID
    assert f(eng._h, d_c.ptr, d_a.ptr, one, one, t._h, 1, 4, 1, None) == ERR_INVALID
    eng.sync()
    assert (d_c.download() == SENTINEL).all()
