"""The second trip of the streaming kernels' grid-stride loops.  Every streaming launcher caps its grid and relies on
`i += gridDim.x * blockDim.x` for the rest; the loop derives unit, polynomial, limb and modulus afresh from the new index.  The other
tests stay at or below every cap (helpers/stream_cases.py lists them), so a unit, limb or polynomial mis-derived in a later trip would
pass them.  Here every launcher gets the smallest shape that gives about one and a half trips -- the total is no multiple of the
stride, so the last trip is partial -- with rows alternating between limbs of different moduli and more than one polynomial where the
call has a polynomial count, outputs prefilled with a sentinel and a sentinel row behind the batch.

References are vectorised: NumPy uint64 where no sum passes 2^64, oracle.cport for products, compared on EVERY word; Python integers
on a sample of 64 columns per row that always holds the first and the last word of every trip.  (The seal cases are small enough for
Python integers throughout.)

Left out: the capped grids of k_ks_mac, k_ks_mac_multi, k_diag_mac and k_sub_scale.  They are reachable only through whole key
switches of more than 4.2 M accumulator words, whose CPU reference takes far longer than a few seconds."""
import ctypes as C

import numpy as np
import pytest

from helpers import stream_cases as S
from oracle import cport as O

pytestmark = pytest.mark.gpu

SENTINEL = 0x5E5E5E5E5E5E5E5E
TOP = 2**64 - 1
P = (1 << 61) - 1
LOGN = S.POINTWISE_LOGN
SUM, RANGE = 1, 2
CLEAN, REPAIRED, UNCORRECTABLE = 0, 1, 2


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


# ---- pointwise batches: a window of three limbs (50, 61, 50 bits) from table limb 1 on, N = 2^12 ------------------------------------
class Batch:
    """operands [n_poly][3][N] (+ a sentinel row), computed once per polynomial count: `a`, `b`, `o` canonical, `aw`, `bw`, `ow` the
    same with any 64-bit word in every fifth column, zeros planted"""

    def __init__(self, F, eng, n_poly, stride):
        self.n_poly, self.limbs, self.start, self.N = n_poly, 3, 1, 1 << LOGN
        self.qs = F.create_moduli(self.N, [61, 50, 61, 50])
        self.t = eng.tables(LOGN, self.qs)
        self.w = self.qs[1:]
        self.rows = n_poly * 3
        self.total = self.rows * self.N
        assert self.total % stride and self.total > stride
        rng = np.random.default_rng(n_poly)
        self.qv = np.array(self.w, dtype=np.uint64).reshape(1, 3, 1)
        shape = (n_poly, 3, self.N)
        canon = lambda: (rng.integers(0, 1 << 62, shape, dtype=np.uint64) % self.qv).astype(np.uint64)
        self.a, self.b, self.o = canon(), canon(), canon()
        for x in (self.a, self.b, self.o):
            x[:, :, 7::97] = 0
            x[:, :, 11::101] = (self.qv - np.uint64(1))
        wild = lambda x: np.where(np.arange(self.N) % 5 == 3, rng.integers(0, TOP, shape, dtype=np.uint64, endpoint=True), x)
        self.aw, self.bw, self.ow = wild(self.a), wild(self.b), wild(self.o)
        # the sampled columns of every row: 64, with the first and last word of every trip
        srng = np.random.default_rng(1000 + n_poly)
        self.cols = np.stack([S.sample_columns(self.N, r * self.N, stride, srng) for r in range(self.rows)])
        first_of_trip_2 = divmod(stride, self.N)
        assert first_of_trip_2[1] in self.cols[first_of_trip_2[0]] and (stride - 1) % self.N in self.cols[(stride - 1) // self.N]
        self.qcol = np.array([self.w[r % 3] for r in range(self.rows)], dtype=object).reshape(-1, 1)

    def with_sentinel(self, x):
        return np.concatenate([x.reshape(self.rows, self.N), np.full((1, self.N), SENTINEL, dtype=np.uint64)])

    def fresh(self):
        return np.full((self.rows + 1, self.N), SENTINEL, dtype=np.uint64)

    def sample(self, x):
        """[rows][64] Python integers of x = [n_poly][3][N]"""
        return np.take_along_axis(x.reshape(self.rows, self.N), self.cols, axis=1).astype(object)

    def check(self, got, want, want_sample):
        """got: [rows + 1][N] as downloaded; want: the vectorised reference, every word; want_sample: Python integers on the sample"""
        assert (got[-1] == SENTINEL).all(), "the call wrote behind its batch"
        body = got[:-1]
        untouched = np.argwhere(body == SENTINEL)
        assert not len(untouched), ("words the call never wrote", untouched[:4].tolist(), len(untouched))
        bad = np.argwhere(body != want.reshape(self.rows, self.N))
        assert not len(bad), (len(bad), bad[:6].tolist())
        assert (np.take_along_axis(body, self.cols, axis=1).astype(object) == want_sample % self.qcol).all()

    def per_limb(self, f, *xs):
        """f(q, flat words of limb l of every operand) -> [n_poly][3][N]"""
        out = np.empty((self.n_poly, 3, self.N), dtype=np.uint64)
        for l, q in enumerate(self.w):
            out[:, l, :] = f(q, *[np.ascontiguousarray(x[:, l, :]).ravel() for x in xs]).reshape(self.n_poly, self.N)
        return out


@pytest.fixture(scope="module")
def batches(F, eng):
    made = {}

    def get(n_poly, stride):
        if n_poly not in made:
            made[n_poly] = Batch(F, eng, n_poly, stride)
        return made[n_poly]
    return get


def _call3(eng, B, f, c, a, b, *tail):
    """upload, run f(ctx, c, a, b, tables, n_poly, limbs, start, *tail), download c"""
    dc, da, db = eng.upload(c), eng.upload(B.with_sentinel(a)), eng.upload(B.with_sentinel(b))
    assert f(eng._h, dc.ptr, da.ptr, db.ptr, B.t._h, B.n_poly, B.limbs, B.start, *tail) == 0
    eng.sync()
    return dc.download().reshape(B.rows + 1, B.N)


@pytest.mark.parametrize("op", ["add", "sub"])
def test_modadd_modsub(F, eng, L, batches, op):
    B = batches(256, S.stride("modadd"))
    ra, rb = B.aw % B.qv, B.bw % B.qv
    want = np.where(ra + rb >= B.qv, ra + rb - B.qv, ra + rb) if op == "add" else np.where(ra >= rb, ra - rb, ra + B.qv - rb)
    sample = B.sample(B.aw) + B.sample(B.bw) if op == "add" else B.sample(B.aw) % B.qcol - B.sample(B.bw) % B.qcol
    got = _call3(eng, B, L.fhe_modadd if op == "add" else L.fhe_modsub, B.fresh(), B.aw, B.bw, None)
    B.check(got, want, sample)


def test_modadd_checked(F, eng, L, batches):
    B = batches(256, S.stride("modadd_checked"))
    s = B.a + B.b
    want = np.where(s >= B.qv, s - B.qv, s)
    dc, da, db = eng.upload(B.fresh()), eng.upload(B.with_sentinel(B.a)), eng.upload(B.with_sentinel(B.b))
    flags = B.t.modadd_checked(dc, da, db, limbs=B.limbs, start=B.start, n_poly=B.n_poly)
    assert flags.shape == (B.rows,) and not flags.any()
    B.check(dc.download().reshape(B.rows + 1, B.N), want, B.sample(B.a) + B.sample(B.b))


@pytest.mark.parametrize("checked", [False, True])
def test_scalar_affine(F, eng, L, batches, checked):
    B = batches(256, S.stride("scalar_affine"))
    rng = np.random.default_rng(5)
    mul, add = [int(rng.integers(1, q)) for q in B.w], [int(rng.integers(1, q)) for q in B.w]
    a = B.a if checked else B.aw
    prod = B.per_limb(lambda q, x: O.modmul(x, np.full(x.size, mul[B.w.index(q)], dtype=np.uint64), q), a)
    addv = np.array(add, dtype=np.uint64).reshape(1, 3, 1)
    want = np.where(prod + addv >= B.qv, prod + addv - B.qv, prod + addv)
    scal = lambda v: np.array([v[r % 3] for r in range(B.rows)], dtype=object).reshape(-1, 1)
    sample = B.sample(a) * scal(mul) + scal(add)
    arr = lambda v: (C.c_uint64 * 3)(*v)
    dc, da = eng.upload(B.fresh()), eng.upload(B.with_sentinel(a))
    if checked:
        flags = B.t.scalar_affine_checked(dc, da, mul=mul, add=add, limbs=B.limbs, start=B.start, n_poly=B.n_poly)
        assert flags.shape == (B.rows,) and not flags.any()
    else:
        assert L.fhe_scalar_affine(eng._h, dc.ptr, da.ptr, arr(mul), arr(add), B.t._h, B.n_poly, B.limbs, B.start, None) == 0
        eng.sync()
    B.check(dc.download().reshape(B.rows + 1, B.N), want, sample)


@pytest.mark.parametrize("elt", [3, 2 * (1 << LOGN) - 1])
def test_automorphism_coefficient_form(F, eng, L, batches, elt):
    """dst[(i k) mod N] = +- src[i] mod q: zeros (which stay zero under the sign) and out-of-range words are planted"""
    B = batches(256, S.stride("automorphism"))
    N = B.N
    i = np.arange(N, dtype=np.uint64)
    j = (i * np.uint64(elt)) & np.uint64(2 * N - 1)
    neg = j >= np.uint64(N)
    r = B.aw % B.qv
    v = np.where(neg & (r != 0), B.qv - r, r)
    want = np.empty_like(v)
    want[:, :, (j & np.uint64(N - 1)).astype(np.int64)] = v
    assert (B.aw == 0).any() and (B.aw >= B.qv).any()
    dst, src = eng.upload(B.fresh()), eng.upload(B.with_sentinel(B.aw))
    assert L.fhe_automorphism(eng._h, dst.ptr, src.ptr, B.t._h, elt, B.n_poly, B.limbs, B.start, None) == 0
    eng.sync()
    got = dst.download().reshape(B.rows + 1, N)
    # Python integers: where the sampled source words went
    flat = B.aw.reshape(B.rows, N)
    for row in range(0, B.rows, 5):
        q = B.w[row % 3]
        for c in B.cols[row]:
            c = int(c)
            jj = c * elt % (2 * N)
            x = int(flat[row, c]) % q
            assert int(got[row, jj % N]) == ((q - x) % q if jj >= N else x), (row, c)
    B.check(got, want, np.take_along_axis(want.reshape(B.rows, N), B.cols, axis=1).astype(object))


def _brev(x, bits):
    r = np.zeros_like(x)
    for _ in range(bits):
        r = (r << np.uint64(1)) | (x & np.uint64(1))
        x = x >> np.uint64(1)
    return r


@pytest.mark.parametrize("checked", [False, True])
@pytest.mark.parametrize("elt", [3, 2 * (1 << LOGN) - 1])
def test_automorphism_ntt_form(F, eng, L, batches, elt, checked):
    """dst[j] = src[j'] with 2 bitrev(j') + 1 = (2 bitrev(j) + 1) k mod 2N, on any words"""
    B = batches(256, S.stride("automorphism_ntt"))
    N = B.N
    j = np.arange(N, dtype=np.uint64)
    e2 = ((np.uint64(2) * _brev(j, LOGN) + np.uint64(1)) * np.uint64(elt)) & np.uint64(2 * N - 1)
    j2 = _brev((e2 - np.uint64(1)) >> np.uint64(1), LOGN).astype(np.int64)
    assert sorted(j2.tolist()) == list(range(N))
    want = B.aw[:, :, j2]
    dst, src = eng.upload(B.fresh()), eng.upload(B.with_sentinel(B.aw))
    if checked:
        from fhe_reliability_gpu_amd.engine import _permute_checked
        flags = _permute_checked(eng, dst, src, LOGN, elt, B.rows)
        assert flags.shape == (B.rows,) and not flags.any()
    else:
        assert L.fhe_automorphism_ntt(eng._h, dst.ptr, src.ptr, LOGN, elt, B.rows, None) == 0
        eng.sync()
    got = dst.download().reshape(B.rows + 1, N)
    flat = B.aw.reshape(B.rows, N)
    brev = lambda x: int(format(x, "0%db" % LOGN)[::-1], 2)
    for row in range(0, B.rows, 5):                                  # Python integers on the sample
        for c in B.cols[row]:
            c = int(c)
            src_col = brev(((2 * brev(c) + 1) * elt % (2 * N) - 1) // 2)
            assert int(got[row, c]) == int(flat[row, src_col]), (row, c)
    assert (got[-1] == SENTINEL).all() and (got[:-1] == want.reshape(B.rows, N)).all()


# ---- modmul: two words per lane --------------------------------------------------------------------------------------------------
def _modmul_case(eng, L, B, acc, checked):
    a, b, o = (B.a, B.b, B.o) if checked else (B.aw, B.bw, B.ow)
    if acc:
        want = B.per_limb(lambda q, z, x, y: O.modmul_acc(z, x, y, q), o, a, b)
        sample = B.sample(a) * B.sample(b) + B.sample(o)
    else:
        want = B.per_limb(lambda q, x, y: O.modmul(x, y, q), a, b)
        sample = B.sample(a) * B.sample(b)
    c = B.with_sentinel(o) if acc else B.fresh()
    if checked:
        dc, da, db = eng.upload(c), eng.upload(B.with_sentinel(a)), eng.upload(B.with_sentinel(b))
        flags = B.t.modmul_checked(dc, da, db, limbs=B.limbs, start=B.start, n_poly=B.n_poly, acc=acc)
        assert flags.shape == (B.rows,) and not flags.any()
        got = dc.download().reshape(B.rows + 1, B.N)
    else:
        got = _call3(eng, B, L.fhe_modmul_acc if acc else L.fhe_modmul, c, a, b, None)
    B.check(got, want, sample)


@pytest.mark.parametrize("checked", [False, True])
@pytest.mark.parametrize("acc", [False, True])
def test_modmul(F, eng, L, batches, acc, checked):
    _modmul_case(eng, L, batches(512, S.stride("modmul")), acc, checked)


@pytest.mark.parametrize("checked", [False, True])
def test_modmul_non_temporal(F, eng, L, batches, checked):
    """just over 8 388 608 words, where the launchers switch to the non-temporal kernels: two whole trips and a third of 4096 words.
    Every word is compared."""
    B = batches(683, S.stride("modmul"))
    assert B.total == 8392704 and B.total * 24 > 192 << 20 and (B.total - 4096) * 24 <= 192 << 20
    _modmul_case(eng, L, B, False, checked)


# ---- tensor product: 97 limbs of 2^16 words, both arithmetic paths ------------------------------------------------------------------
@pytest.fixture(scope="module")
def tensor_case(F, eng):
    logn, limbs = 16, 97
    N = 1 << logn
    assert S.trips("tensor", limbs * N) == (2, True)
    qs = F.create_moduli(N, [50 if l % 2 == 0 else 61 for l in range(limbs)])
    t = eng.tables(logn, qs)
    assert set(t.paths) == {0, 1}
    rng = np.random.default_rng(97)
    qv = np.array(qs, dtype=np.uint64).reshape(-1, 1)
    host = [(rng.integers(0, 1 << 62, (limbs, N), dtype=np.uint64) % qv).astype(np.uint64) for _ in range(4)]
    a0, a1, b0, b1 = host
    want = [np.empty((limbs, N), dtype=np.uint64) for _ in range(3)]
    for l, q in enumerate(qs):                                       # every word, from the C oracle
        want[0][l] = O.modmul(a0[l], b0[l], q)
        want[1][l] = O.modmul_acc(O.modmul(a0[l], b1[l], q), a1[l], b0[l], q)
        want[2][l] = O.modmul(a1[l], b1[l], q)
    srng = np.random.default_rng(98)
    cols = np.stack([S.sample_columns(N, l * N, S.stride("tensor"), srng) for l in range(limbs)])
    assert 0 in cols[64] and N - 1 in cols[63]                       # the first word of the second trip and the word before it
    g = lambda x: np.take_along_axis(x, cols, axis=1).astype(object)
    qcol = np.array(qs, dtype=object).reshape(-1, 1)
    sample = [g(a0) * g(b0) % qcol, (g(a0) * g(b1) + g(a1) * g(b0)) % qcol, g(a1) * g(b1) % qcol]
    for k in range(3):
        assert (g(want[k]) == sample[k]).all()
    return t, limbs, N, [eng.upload(h) for h in host], want


@pytest.mark.parametrize("checked", [False, True])
def test_tensor_product(F, eng, L, tensor_case, checked):
    t, limbs, N, ops, want = tensor_case
    d = [eng.upload(np.full((limbs + 1, N), SENTINEL, dtype=np.uint64)) for _ in range(3)]
    args = [eng._h, d[0].ptr, d[1].ptr, d[2].ptr, ops[0].ptr, ops[1].ptr, ops[2].ptr, ops[3].ptr, t._h, limbs, 0]
    if checked:
        flags = eng.upload(np.full((3 * limbs + 1) // 2, 0xA5A5A5A5DEADBEEF, dtype=np.uint64))
        assert L.fhe_tensor_product_checked(*args, flags.ptr, None) == 0
    else:
        assert L.fhe_tensor_product(*args, None) == 0
    eng.sync()
    for k in range(3):
        got = d[k].download().reshape(limbs + 1, N)
        assert (got[-1] == SENTINEL).all(), "the call wrote behind its batch"
        bad = np.argwhere(got[:-1] != want[k])
        assert not len(bad), (k, len(bad), bad[:6].tolist())
    if checked:
        assert not flags.download().view(np.uint32)[:3 * limbs].any()


# ---- one lane per column: fast base conversion, Garner, Hadamard ------------------------------------------------------------------
def _column_sample(n, seed):
    return S.sample_columns(n, 0, S.stride("bconv_fast"), np.random.default_rng(seed))


@pytest.mark.parametrize("checked", [False, True])
def test_fast_base_conversion(F, eng, checked):
    N = S.COLUMNS
    qs = F.create_moduli(1 << 10, [50, 61, 50, 61, 30])
    mi, mo = qs[:2], qs[2:]
    rng = np.random.default_rng(21)
    x = np.stack([rng.integers(0, p, N, dtype=np.uint64) for p in mi])
    want = np.ascontiguousarray(O.bconv_fast(x, mi, mo).T)                    # [k][N], the unreduced sums
    cols = _column_sample(N, 22)
    assert {(1 << 20) - 1, 1 << 20, N - 1, 0} <= set(cols.tolist())
    for o, q in enumerate(mo):                                               # Python integers on the sample
        coef = []
        for j, p in enumerate(mi):
            hat = 1
            for l, pl in enumerate(mi):
                hat *= pl if l != j else 1
            coef.append(hat % q * (pow(hat % p, -1, p) % q) % q)
        for c in cols:
            assert int(want[o, c]) == sum(int(x[j, c]) % q * coef[j] % q for j in range(len(mi)))
    bc = F.BaseConv(eng, mi, mo)
    d_in, d_out = eng.upload(x), eng.upload(np.full((len(mo) + 1, N), SENTINEL, dtype=np.uint64))
    if checked:
        flags = bc.fast_checked(d_out, d_in, N)
        assert flags.shape == (len(mo),) and not flags.any()
    else:
        bc.fast(d_out, d_in, N)
        eng.sync()
    got = d_out.download().reshape(len(mo) + 1, N)
    assert (got[-1] == SENTINEL).all() and (got[:-1] == want).all()


def test_crt_garner(F, eng, L):
    N = S.COLUMNS
    mods = F.create_moduli(1 << 10, [61, 50, 61, 50])                        # (the prefix products wrap 128 bits at the fourth limb)
    rng = np.random.default_rng(31)
    res = np.stack([rng.integers(0, p, N, dtype=np.uint64) for p in mods])
    want_lo, want_hi = O.crt_garner(res, mods)
    cols = _column_sample(N, 32)
    s_lo, s_hi = S.garner_python(res[:, cols], mods)
    assert (s_lo == want_lo[cols]).all() and (s_hi == want_hi[cols]).all()
    d = eng.upload(res)
    lo, hi = (eng.upload(np.full(N + 8, SENTINEL, dtype=np.uint64)) for _ in range(2))
    mod = np.array(mods, dtype=np.uint64)
    assert L.fhe_crt_garner(eng._h, lo.ptr, hi.ptr, d.ptr, mod.ctypes.data_as(C.POINTER(C.c_uint64)), len(mods), N, None) == 0
    eng.sync()
    for got, want in ((lo.download(), want_lo), (hi.download(), want_hi)):
        assert (got[N:] == SENTINEL).all() and (got[:N] == want).all()


def test_bsgs_hadamard_mod(F, eng, L):
    k, bs = S.HADAMARD_K, S.HADAMARD_BS
    q = F.create_moduli(1 << 10, [61])[0]
    rng = np.random.default_rng(41)
    M, v = (rng.integers(0, TOP, (k, bs), dtype=np.uint64, endpoint=True) for _ in range(2))
    want = O.bsgs_hadamard_mod(M, v, q)
    cols = S.sample_columns(k * bs, 0, S.stride("bsgs_hadamard"), np.random.default_rng(42))
    assert {(1 << 20) - 1, 1 << 20, k * bs - 1} <= set(cols.tolist())
    for o in cols:
        i, e = divmod(int(o), bs)
        assert int(want[o]) == sum(int(M[(j - i) % k, e]) * int(v[j, e]) for j in range(k)) % q
    dM, dv = eng.upload(M), eng.upload(v)
    y = eng.upload(np.full(k * bs + 8, SENTINEL, dtype=np.uint64))
    assert L.fhe_bsgs_hadamard(eng._h, y.ptr, dM.ptr, dv.ptr, k, bs, q, None) == 0
    eng.sync()
    got = y.download()
    assert (got[k * bs:] == SENTINEL).all() and (got[:k * bs] == want).all()


# ---- seals: one workgroup per (row, chunk) job -------------------------------------------------------------------------------------
def _py_sums(x):
    """[rows][3] Python integers: S0, S1, S2 of the rows of x modulo 2^61 - 1"""
    rows = np.asarray(x).astype(object)
    w = np.arange(1, rows.shape[1] + 1).astype(object)
    return np.stack([rows.sum(axis=1) % P, (rows * w).sum(axis=1) % P, (rows * w * w).sum(axis=1) % P], axis=1)


def _flip(eng, L, d, idx, bit):
    assert L.fhe_flip_bit(eng._h, d.ptr, int(idx), int(bit), None) == 0


SEAL_BITS = [50, 61, 50, 61, 50, 61, 50]


def _seal_rows(F, eng, logn, n_poly, seed):
    N = 1 << logn
    qs = F.create_moduli(N, SEAL_BITS)
    t = eng.tables(logn, qs)
    rng = np.random.default_rng(seed)
    qv = np.array(qs * n_poly, dtype=np.uint64).reshape(-1, 1)
    x = (rng.integers(0, 1 << 62, (n_poly * 7, N), dtype=np.uint64) % qv) >> np.uint64(1)        # below q / 2: a low flipped bit stays in the window
    return t, qs, x


def _seal_verify_locate(eng, L, t, x, n_poly, flips):
    """seals and locators == Python, a clean verify, and `flips` = [(row, word)] raises exactly those rows"""
    rows, N = x.shape
    kw = dict(limbs=7, start=0, n_poly=n_poly)
    d = eng.upload(x)
    sums = _py_sums(x)
    seal = t.seal(d, **kw)
    assert (seal.download().reshape(rows, 2).astype(object) == sums[:, :2]).all()
    assert (t.seal_locator(d, **kw).download().astype(object) == sums[:, 2]).all()
    assert not t.seal_verify(d, seal, **kw).any()
    for r, j in flips:
        _flip(eng, L, d, r * N + j, 3)
    flags = t.seal_verify(d, seal, **kw)
    want = np.zeros(rows, dtype=np.uint32)
    want[[r for r, _ in flips]] = SUM
    assert (flags == want).all(), (np.nonzero(flags)[0].tolist(), sorted(r for r, _ in flips))
    # the locator of the changed rows moves with the word, every other one stays
    y = x.copy()
    for r, j in flips:
        y[r, j] ^= np.uint64(8)
    assert (t.seal_locator(d, **kw).download().astype(object) == _py_sums(y)[:, 2]).all()
    eng.check()


def test_seal_verify_locator_12285_rows(F, eng, L):
    """N = 2: 7 limbs x 1755 polynomials, one job per row, 8192 in the first trip"""
    n_poly = 1755
    t, qs, x = _seal_rows(F, eng, 1, n_poly, 51)
    assert S.trips("seal", x.shape[0]) == (2, True)
    flips = [(0, 0), (8191, 1), (8192, 0), (8193, 1), (10000, 0), (12284, 1), (4097, 0)]
    _seal_verify_locate(eng, L, t, x, n_poly, flips)


def test_seal_verify_locator_two_chunks(F, eng, L):
    """N = 2^14: 7 rows of two chunks each; a flipped word on either side of the chunk boundary"""
    t, qs, x = _seal_rows(F, eng, 14, 1, 52)
    _seal_verify_locate(eng, L, t, x, 1, [(1, (1 << 13) - 1), (4, 1 << 13), (6, (1 << 14) - 1)])


def test_seal_repair_3073_rows(F, eng, L):
    """N = 2, 3073 rows (439 polynomials of 7 limbs), 2048 in the first trip: every row corrupted in one word, but for a few clean rows
    (the loop's `continue`, also in the second trip) and a few rows with both words corrupted"""
    n_poly = 439
    t, qs, x = _seal_rows(F, eng, 1, n_poly, 53)
    rows, N = x.shape
    assert rows == 3073 and S.trips("seal_repair", rows) == (2, True)
    kw = dict(limbs=7, start=0, n_poly=n_poly)
    d_clean = eng.upload(x)
    seal, loc = t.seal(d_clean, **kw), t.seal_locator(d_clean, **kw)
    sums = _py_sums(x)
    assert (seal.download().reshape(rows, 2).astype(object) == sums[:, :2]).all() and (loc.download().astype(object) == sums[:, 2]).all()
    clean = {5, 2047, 2048, 2500, 3072 - 1}
    double = {9, 1000, 2049, 3000}
    y = x.copy()
    want_rep = np.zeros((rows, 4), dtype=np.uint64)
    for r in range(rows):
        q = qs[r % 7]
        if r in clean:
            continue
        if r in double:
            y[r] ^= np.uint64(8)                                      # both words, in the window: d1 d2 != 0
            want_rep[r, 0] = UNCORRECTABLE
            continue
        j, bit = r & 1 if r % 3 else 1 - (r & 1), r % 60              # bits up to 59: a 50-bit limb's word may be pushed past q
        y[r, j] ^= np.uint64(1 << bit)
        want_rep[r, 0], want_rep[r, 1], want_rep[r, 2], want_rep[r, 3] = REPAIRED, j, y[r, j], x[r, j]
    assert (y[sorted(double)] < np.array([qs[r % 7] for r in sorted(double)], dtype=np.uint64).reshape(-1, 1)).all()
    assert any(int(y[r, j]) >= qs[r % 7] for r in range(rows) for j in range(2)), "no word pushed past q"
    assert {r >= 2048 for r in clean} == {r >= 2048 for r in double} == {False, True}
    d = eng.upload(y)
    flags, report = t.seal_repair(d, seal, loc, **kw)
    bad = np.nonzero((report != want_rep).any(axis=1))[0]
    assert not len(bad), (len(bad), bad[:6].tolist(), report[bad[:6]].tolist(), want_rep[bad[:6]].tolist())
    want_flags = np.zeros(rows, dtype=np.uint32)
    want_flags[sorted(double)] = SUM
    assert (flags == want_flags).all()
    restored = x.copy()
    restored[sorted(double)] = y[sorted(double)]
    assert (d.download().reshape(rows, N) == restored).all()
    eng.check()
