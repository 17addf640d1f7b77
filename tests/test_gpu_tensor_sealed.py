"""The sealed tensor product on the GPU: operands verified on the load that multiplies them, results sealed from the registers that
are stored.  Words are held against KeySwitch.tensor and against Python-integer products, seals against Python-integer sums computed
here from the host arrays.

Shapes (logn, L, limb kinds): (5, 2) a row shorter than a workgroup; (10, 3) mixed 50 / 61-bit primes, both arithmetic paths in one
call; (13, 2) exactly one chunk per row; (14, 2) 61-bit, two chunks per row, where a word's weight is its index in the row and not
in the chunk; and, through the C ABI, (1, 1) with 3 * cap + 1 polynomials: the job loop takes a fourth trip on less than 1 MiB per
operand."""
import numpy as np
import pytest

from helpers.checked_plan import checked_plan
from helpers.sealed_case import P, case_cache, flip, py_seals, raised

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
SUM, RANGE = 1, 2
GARBAGE = 0x5A5A5A5A5A5A5A5A
GRID_CAP = 8192                 # TENSOR_SEAL_GRID_CAP of ntt_launch.hpp: workgroups of the job loop at most
SHAPES = [(5, 2, "50"), (10, 3, "mixed"), (13, 2, "50"), (14, 2, "61")]
NAMES = ("a0", "a1", "b0", "b1")
ENTERS = {"a0": (0, 1), "a1": (1, 2), "b0": (0, 1), "b1": (1, 2)}      # the parts an operand enters


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


def py_tensor(ops, qs):
    """fhe_tensor_product's words of ops = 4 x [rows][N] (any 64-bit words), row r modulo qs[r]: Python integers"""
    a0, a1, b0, b1 = (np.asarray(x).astype(object) for x in ops)
    q = np.array([int(v) for v in qs], dtype=object)[:, None]
    return [((a0 * b0) % q).astype(np.uint64), ((a0 * b1 + a1 * b0) % q).astype(np.uint64), ((a1 * b1) % q).astype(np.uint64)]


def spots_of(logn):
    """first and last word of a row, and both sides of the chunk edge (of the row's middle below two chunks)"""
    N = 1 << logn
    mid = 1 << 13 if logn > 13 else N // 2
    return [0, mid - 1, mid, N - 1]


class Case:
    """a plan, seeded operands on the host and on the device, their seals, and the clean product"""

    def __init__(self, F, eng, logn, L, kind):
        self.logn, self.L, self.N = logn, L, 1 << logn
        self.qs, self.t, self.ks, self.ab, rng = checked_plan(F, eng, logn, L, 1, L, kind, 1000 * logn + L)
        self.q = self.qs[:L]
        self.spots = spots_of(logn)
        self.ops = [np.stack([rng.integers(0, q, self.N, dtype=np.uint64) for q in self.q]) for _ in range(4)]
        for o, x in enumerate(self.ops):
            x[:, self.spots] = [[1000 * (o + 1) + 16 * s + 32 * r + 5 for s in range(4)] for r in range(L)]      # bit 3 flips stay below q
        self.ops[1][L - 1, 7 % self.N] = self.q[L - 1] - 1
        self.ops[3][L - 1, 7 % self.N] = self.q[L - 1] - 1
        self.d = [eng.upload(x) for x in self.ops]
        self.seals = [self.t.seal(v, limbs=L) for v in self.d]
        for v, s in zip(self.ops, self.seals):
            assert s.download().tolist() == py_seals(v)
        self.clean = [x.download() for x in self.ks.tensor(*self.d)]
        want = py_tensor(self.ops, self.q)
        assert all((g == w).all() for g, w in zip(self.clean, want))
        self.clean_seals = [py_seals(w) for w in self.clean]


@pytest.fixture(scope="module")
def cases(F, eng):
    return case_cache(lambda shape: Case(F, eng, *shape))


def words(d):
    return [x.download() for x in d]


@pytest.mark.parametrize("shape", SHAPES)
def test_clean_words_flags_and_output_seals(F, eng, cases, shape):
    c = cases(shape)
    ks, L = c.ks, c.L
    lay = ks.tensor_sealed_layout()
    assert [lay[n][0] for n in NAMES + ("tensor",)] == [0, L, 2 * L, 3 * L, 4 * L] and lay["total"] == 7 * L
    d0, d1, d2, so, fl = ks.tensor_sealed(*c.d, seals=c.seals)      # the flag buffer starts out as garbage (engine._flag_buffer)
    assert sorted(fl) == sorted(NAMES + ("tensor",)) and fl["tensor"].shape == (L, 3)
    assert raised(fl) == []
    got = words((d0, d1, d2))
    assert all((g == w).all() for g, w in zip(got, c.clean))
    for s, dev, want in zip(so, (d0, d1, d2), c.clean_seals):
        assert s.download().tolist() == want
        assert s.download().tolist() == c.t.seal(dev, limbs=L).download().tolist()
    # without output seals: the other instantiation, the same words
    d0, d1, d2, so, fl = ks.tensor_sealed(*c.d, seals=c.seals, seal_out=False)
    assert so is None and raised(fl) == [] and all((g == w).all() for g, w in zip(words((d0, d1, d2)), c.clean))
    # squaring: a and b the same buffers
    sq = ks.tensor_sealed(c.d[0], c.d[1], c.d[0], c.d[1], seals=[c.seals[0], c.seals[1], c.seals[0], c.seals[1]])
    want = py_tensor([c.ops[0], c.ops[1], c.ops[0], c.ops[1]], c.q)
    assert raised(sq[4]) == [] and all((g == w).all() for g, w in zip(words(sq[:3]), want))
    assert [s.download().tolist() for s in sq[3]] == [py_seals(w) for w in want]
    # inputs untouched
    assert all((dv.download() == v).all() for dv, v in zip(c.d, c.ops))
    eng.check()


@pytest.mark.parametrize("shape", SHAPES)
def test_an_output_may_be_an_operands_buffer(F, eng, cases, shape):
    from fhe_reliability_gpu_amd._lib import check, lib, vp
    c = cases(shape)
    L = c.L
    # d0 onto a0, d1 onto b1, d2 onto a1
    a0, a1, b0, b1 = (eng.upload(x) for x in c.ops)
    so = [eng.alloc(2 * L) for _ in range(3)]
    flags = eng.upload(np.full((7 * L + 1) // 2, GARBAGE, dtype=np.uint64))
    sin, sout = (vp * 4)(*[s.ptr for s in c.seals]), (vp * 3)(*[s.ptr for s in so])
    check(lib.fhe_tensor_product_sealed(eng._h, a0.ptr, b1.ptr, a1.ptr, a0.ptr, a1.ptr, b0.ptr, b1.ptr, c.t._h, 1, L, 0, sin, sout, flags.ptr, None))
    assert not flags.download().view(np.uint32)[:7 * L].any()
    for dev, want, s, ws in zip((a0, b1, a1), c.clean, so, c.clean_seals):
        assert (dev.download().reshape(L, c.N) == want).all()
        assert s.download().reshape(L, 2).tolist() == ws
    eng.check()


@pytest.mark.parametrize("shape", SHAPES)
def test_changes_at_rest_raise_their_row_and_the_product_is_that_of_the_words_as_they_are(F, eng, cases, shape):
    c = cases(shape)
    ks, L, N = c.ks, c.L, c.N

    def run(ops_dev, ops_host, seals, want_flags):
        d0, d1, d2, so, fl = ks.tensor_sealed(*ops_dev, seals=seals)
        assert {(n, r): int(fl[n][r]) for n, r in raised(fl)} == want_flags, (raised(fl), want_flags)
        assert not fl["tensor"].any()                      # the identity holds on the operand as it is
        want = py_tensor(ops_host, c.q)
        assert all((g == w).all() for g, w in zip(words((d0, d1, d2)), want))
        assert [s.download().tolist() for s in so] == [py_seals(w) for w in want]

    for o, name in enumerate(NAMES):
        row = o % L
        # one word, at each spot
        for j in c.spots:
            flip(eng, c.d[o], row * N + j, 3)
            try:
                host = [x.copy() for x in c.ops]
                host[o][row, j] ^= np.uint64(8)
                run(c.d, host, c.seals, {(name, row): SUM})
            finally:
                flip(eng, c.d[o], row * N + j, 3)
        # x -> x + p: no sum moves, the window alone sees it
        host = [x.copy() for x in c.ops]
        host[o][row, c.spots[1]] += np.uint64(P)
        dev = list(c.d)
        dev[o] = eng.upload(host[o])
        d0, d1, d2, so, fl = ks.tensor_sealed(*dev, seals=c.seals)
        assert {(n, r): int(fl[n][r]) for n, r in raised(fl) if n != "tensor"} == {(name, row): RANGE}
        assert all((g == w).all() for g, w in zip(words((d0, d1, d2)), py_tensor(host, c.q)))
        # two words of one row by +d and -d: S0 does not move
        host = [x.copy() for x in c.ops]
        host[o][row, c.spots[0]] += np.uint64(3)
        host[o][row, c.spots[3]] -= np.uint64(3)
        assert py_seals(host[o])[row][0] == py_seals(c.ops[o])[row][0]
        dev = list(c.d)
        dev[o] = eng.upload(host[o])
        run(dev, host, c.seals, {(name, row): SUM})
        # a changed seal word
        s = c.seals[o].download().copy()
        s[row, 1] ^= np.uint64(1 << 20)
        seals = list(c.seals)
        seals[o] = eng.upload(s)
        run(c.d, c.ops, seals, {(name, row): SUM})
    assert all((dv.download() == v).all() for dv, v in zip(c.d, c.ops))
    assert raised(ks.tensor_sealed(*c.d, seals=c.seals)[4]) == []
    eng.check()


@pytest.mark.parametrize("shape", SHAPES)
def test_a_fault_on_the_load_raises_the_operands_row_and_leaves_memory_clean(F, eng, cases, shape):
    c = cases(shape)
    ks, L, N = c.ks, c.L, c.N
    for o, name in enumerate(NAMES):
        row = (o + 1) % L
        for j in (c.spots[0], c.spots[2], c.spots[3]):
            eng.inject_fault_tensor_sealed(o, row, j, 3)
            d0, d1, d2, so, fl = ks.tensor_sealed(*c.d, seals=c.seals)
            assert {(n, r): int(fl[n][r]) for n, r in raised(fl)} == {(name, row): SUM}, (name, j, raised(fl))
            assert all((dv.download() == v).all() for dv, v in zip(c.d, c.ops))      # memory is clean
            got = words((d0, d1, d2))
            for part in range(3):
                diff = np.argwhere(got[part] != c.clean[part]).tolist()
                assert diff == ([[row, j]] if part in ENTERS[name] else []), (name, j, part)
            host = [x.copy() for x in c.ops]
            host[o][row, j] ^= np.uint64(8)
            want = py_tensor(host, c.q)
            assert all((g == w).all() for g, w in zip(got, want))
            assert [s.download().tolist() for s in so] == [py_seals(w) for w in want]
            # one shot
            d0, d1, d2, so, fl = ks.tensor_sealed(*c.d, seals=c.seals)
            assert raised(fl) == [] and all((g == w).all() for g, w in zip(words((d0, d1, d2)), c.clean))
    # out of the window on the load: both bits, and the parts it enters cannot be checked
    eng.inject_fault_tensor_sealed(1, 0, 1, 63)
    fl = ks.tensor_sealed(*c.d, seals=c.seals)[4]
    assert int(fl["a1"][0]) == SUM | RANGE and fl["tensor"][0].tolist() == [0, 4, 4]
    assert [(n, r) for n, r in raised(fl) if n != "tensor"] == [("a1", 0)]
    eng.check()


@pytest.mark.parametrize("shape", SHAPES)
def test_the_pointwise_hook_raises_d1_and_null_seals_are_skipped(F, eng, cases, shape):
    from fhe_reliability_gpu_amd._lib import check, lib
    c = cases(shape)
    ks, L, N = c.ks, c.L, c.N
    row, j = L - 1, c.spots[2]
    for point in (0, 1, 2, 3):
        check(lib.fhe_ctx_inject_fault_pointwise(eng._h, point, row * N + j, 3))
        d0, d1, d2, so, fl = ks.tensor_sealed(*c.d, seals=c.seals)
        # a flipped result word (point 2) always changes it; at the other points the reduction may absorb the flip, and then
        # nothing is raised (tests/test_gpu_pointwise_checked.py): no seal word either way
        changed = np.argwhere(d1.download() != c.clean[1]).tolist()
        assert changed == [[row, j]] or (point != 2 and changed == []), (point, changed)
        assert raised(fl) == ([("tensor", 3 * row + 1)] if changed else []), (point, raised(fl))
        assert so[1].download().tolist() == py_seals(d1.download())      # the digest is of the registers stored
        assert (d0.download() == c.clean[0]).all() and (d2.download() == c.clean[2]).all()
        assert raised(ks.tensor_sealed(*c.d, seals=c.seals)[4]) == []     # one shot
    # null seals: not compared
    flip(eng, c.d[0], 0 * N + c.spots[0], 3)
    flip(eng, c.d[3], (L - 1) * N + c.spots[3], 3)
    try:
        fl = ks.tensor_sealed(*c.d, seals=c.seals)[4]
        assert raised(fl) == [("a0", 0), ("b1", L - 1)]
        assert raised(ks.tensor_sealed(*c.d, seals=[None, c.seals[1], c.seals[2], c.seals[3]])[4]) == [("b1", L - 1)]
        assert raised(ks.tensor_sealed(*c.d, seals=[None, c.seals[1], c.seals[2], None])[4]) == []
        assert raised(ks.tensor_sealed(*c.d)[4]) == []
    finally:
        flip(eng, c.d[0], 0 * N + c.spots[0], 3)
        flip(eng, c.d[3], (L - 1) * N + c.spots[3], 3)
    # the window is checked all the same
    host = c.ops[2].copy()
    host[0, 1] = c.q[0]
    fl = ks.tensor_sealed(c.d[0], c.d[1], eng.upload(host), c.d[3])[4]
    assert [(n, r, int(fl[n][r])) for n, r in raised(fl) if n != "tensor"] == [("b0", 0, RANGE)]
    eng.check()


def test_refusals_are_statuses_and_launch_nothing(F, eng, cases):
    from fhe_reliability_gpu_amd._lib import check, lib, vp
    c = cases(SHAPES[1])
    L, N = c.L, c.N
    d = [eng.alloc(L * N + 2) for _ in range(3)]
    sin = (vp * 4)(*[s.ptr for s in c.seals])
    so = [eng.alloc(2 * L) for _ in range(3)]
    sout = (vp * 3)(*[s.ptr for s in so])
    n_words = (7 * L + 1) // 2 + 8
    ptr = lambda x, off=0: x.ptr.value + off if x is not None else None

    def call(flags, dd=None, ops=None, limbs=L, start=0):
        dd = [ptr(x) for x in d] if dd is None else dd
        ops = [ptr(x) for x in c.d] if ops is None else ops
        return lib.fhe_tensor_product_sealed(eng._h, dd[0], dd[1], dd[2], ops[0], ops[1], ops[2], ops[3], c.t._h, 1, limbs, start, sin, sout, flags, None)

    def refused(status, why, **kw):
        fl = eng.upload(np.full(n_words, GARBAGE, dtype=np.uint64))
        assert call(fl.ptr, **kw) == status and why in lib.fhe_last_error().decode(), (why, lib.fhe_last_error())
        assert (fl.download() == GARBAGE).all()      # nothing launched, not even the clearing of the flags

    fl = eng.upload(np.full(n_words, GARBAGE, dtype=np.uint64))
    assert call(fl.ptr) == 0 and not fl.download().view(np.uint32)[:7 * L].any()
    for i in range(3):      # a misaligned output, a misaligned operand
        dd = [ptr(x) for x in d]
        dd[i] += 8
        refused(INVALID, "16-byte", dd=dd)
    for i in range(4):
        ops = [ptr(x) for x in c.d]
        ops[i] += 8
        refused(INVALID, "16-byte", ops=ops)
        ops[i] = None
        refused(INVALID, "null", ops=ops)
    dd = [ptr(x) for x in d]
    dd[1] = None
    refused(INVALID, "null", dd=dd)
    assert call(None) == INVALID
    refused(INVALID, "limb range", limbs=len(c.qs) + 1)
    refused(INVALID, "limb range", start=len(c.qs), limbs=1)
    # a hook outside the call that takes it: refused, and gone afterwards
    for bad in ((0, L, 0, 3), (3, 0, N, 3)):
        eng.inject_fault_tensor_sealed(*bad)
        refused(INVALID, "outside the call")
        assert call(fl.ptr) == 0 and not fl.download().view(np.uint32)[:7 * L].any()
    check(lib.fhe_ctx_inject_fault_pointwise(eng._h, 2, L * N, 3))
    refused(INVALID, "outside")
    # the setter
    for bad in ((4, 0, 0, 0), (0, -1, 0, 0), (0, 0, -1, 0), (0, 0, 0, 64), (0, 0, 0, -1)):
        assert lib.fhe_ctx_inject_fault_tensor_sealed(eng._h, *bad) == INVALID
    eng.inject_fault_tensor_sealed(2, 0, 0, 3)
    eng.inject_fault_tensor_sealed(-1)                      # disarmed
    assert call(fl.ptr) == 0 and not fl.download().view(np.uint32)[:7 * L].any()
    # a refused call takes the hook with it
    eng.inject_fault_tensor_sealed(2, 0, 0, 3)
    refused(INVALID, "null", dd=dd)
    assert call(fl.ptr) == 0 and not fl.download().view(np.uint32)[:7 * L].any()
    eng.check()


def test_the_job_loop_takes_a_fourth_trip(F, eng):
    from fhe_reliability_gpu_amd._lib import check, lib, vp
    logn, N = 1, 2
    n_poly = 3 * GRID_CAP + 1
    qs = F.create_moduli(N, [50])
    t = eng.tables(logn, qs)
    q = qs[0]
    rng = np.random.default_rng(31)
    ops = [rng.integers(0, q, (n_poly, N), dtype=np.uint64) for _ in range(4)]
    assert ops[0].nbytes < 1 << 20
    dev = [eng.upload(x) for x in ops]
    seals = [t.seal(v, limbs=1, n_poly=n_poly) for v in dev]
    d = [eng.alloc(n_poly * N) for _ in range(3)]
    so = [eng.alloc(2 * n_poly) for _ in range(3)]
    sin, sout = (vp * 4)(*[s.ptr for s in seals]), (vp * 3)(*[s.ptr for s in so])
    lay = (np.ctypeslib.ctypes.c_int * 6)()
    check(lib.fhe_tensor_product_sealed_layout(n_poly, 1, lay))
    R = n_poly
    assert list(lay) == [0, R, 2 * R, 3 * R, 4 * R, 7 * R]

    def call(operands):
        flags = eng.upload(np.full((7 * R + 1) // 2, GARBAGE, dtype=np.uint64))
        check(lib.fhe_tensor_product_sealed(eng._h, d[0].ptr, d[1].ptr, d[2].ptr, *[x.ptr for x in operands], t._h, n_poly, 1, 0, sin, sout, flags.ptr, None))
        return flags.download().view(np.uint32)[:7 * R].copy()

    fl = call(dev)
    assert not fl.any()
    want = py_tensor(ops, [q] * n_poly)
    for x, w, s in zip(d, want, so):
        got = x.download().reshape(n_poly, N)
        assert (got == w).all()
        sums = s.download().reshape(n_poly, 2)
        for r in (0, GRID_CAP - 1, GRID_CAP, 3 * GRID_CAP - 1, 3 * GRID_CAP):
            assert sums[r].tolist() == py_seals(w[r:r + 1])[0], r
        x.shape = (n_poly, N)
        assert (sums == t.seal(x, limbs=1, n_poly=n_poly).download().reshape(n_poly, 2)).all()
    # the last row is the fourth trip of workgroup 0: a word changed there raises exactly that row of that operand
    for o, r in ((0, 3 * GRID_CAP), (3, 2 * GRID_CAP + 5)):
        host = ops[o].copy()
        host[r, 1] ^= np.uint64(1)
        operands = list(dev)
        operands[o] = eng.upload(host)
        fl = call(operands)
        assert np.flatnonzero(fl).tolist() == [o * R + r] and int(fl[o * R + r]) == SUM
    eng.check()
