"""The FP64 transform on the inputs of tests/helpers/ntt_worst_case.py -- ladders, pulses and the soak patterns, built for the
largest 50-bit prime and a 30-bit one -- in every form the engine has: the default, the LDS-resident pass, the fused launch, the
packed hand-off, the fused product and the checked calls.  The natural-order four-step takes the vectors built for its own table
(tests/helpers/gs_worst_case.py; tests/test_gpu_natural_order_worst_case.py holds the rest of that route).  Every comparison is ==
against the oracle.

Sizes: 2^4, 2^9, 2^12 (one, two, three register steps), 2^13 / 2^14 (resident, fused), 2^16 (packed, two-step rows), 2^17
(three-step rows, last fused size), 2^18 (a fourth stretch of forward stages)."""
import numpy as np
import pytest

from helpers import gs_worst_case as G
from helpers import ntt_worst_case as W

pytestmark = pytest.mark.gpu

SIZES = [4, 9, 12, 13, 14, 16, 17, 18]
Q61 = 2305843009211596801


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


_CASES = {}


def _case(O, logn):
    """Every family for both primes, polynomial p = (vector for the 50-bit limb, vector for the 30-bit limb), with the oracle's
    images: computed once per size, shared, never modified."""
    if logn not in _CASES:
        limbs = [W.Limb(logn, 50), W.Limb(logn, 30)]
        names, cols, inv_names, inv_cols = [], [], [], []
        for k, L in enumerate(limbs):
            col, icol = [], []
            for s0, K, canonical in W.forward_stretches(logn) + (W.forward_stretches(16, canonical_at=(8,))[2:3] if logn == 16 else []):
                col.append((f"ladder{s0}+{K}", W.forward_ladder(L, s0, K, canonical)[0]))
            for t in range(logn):
                v = W.inverse_pulse(L, t)[0]
                col.append((f"ipulse{t}", v))
                icol.append((f"ipulse{t}", v))
                col.append((f"fpulse{t}", W.forward_pulse(L, t)[0]))
            for name, v, *_ in W.soak_patterns(L):
                col.append((name, v))
                icol.append((name, v))
            cols.append([v for _, v in col])
            inv_cols.append([v for _, v in icol])
            names, inv_names = [n for n, _ in col], [n for n, _ in icol]
        qs = [L.q for L in limbs]
        rps = np.stack([L.rp for L in limbs])
        data = np.stack([np.stack([cols[0][p], cols[1][p]]) for p in range(len(names))])
        inv_data = np.stack([np.stack([inv_cols[0][p], inv_cols[1][p]]) for p in range(len(inv_names))])
        P, PI = len(names), len(inv_names)
        tile = lambda x, n: np.tile(np.asarray(x), (n,) + (1,) * (np.asarray(x).ndim - 1))
        fwd = O.nwt_forward_batch(data.reshape(2 * P, -1), tile(qs, P), tile(rps, P)).reshape(data.shape)
        inv = O.nwt_inverse_batch(inv_data.reshape(2 * PI, -1), tile(qs, PI), tile(rps, PI)).reshape(inv_data.shape)
        for a in (data, fwd, inv_data, inv):
            a.setflags(write=False)
        _CASES[logn] = dict(limbs=limbs, qs=qs, names=names, data=data, fwd=fwd, inv_names=inv_names, inv_data=inv_data, inv=inv)
    return _CASES[logn]


def _bad(names, got, want):
    return [(names[p], l) for p in range(got.shape[0]) for l in range(got.shape[1]) if not (got[p, l] == want[p, l]).all()]


def _transforms(eng, t, c, what):
    P, PI = len(c["names"]), len(c["inv_names"])
    d = eng.upload(c["data"])
    t.forward(d, n_poly=P)
    assert _bad(c["names"], d.download(), c["fwd"]) == [], what
    t.inverse(d, n_poly=P)                       # the inverse of the oracle's image gives the input back
    assert _bad(c["names"], d.download(), c["data"]) == [], what
    d.free()
    d = eng.upload(c["inv_data"])
    t.inverse(d, n_poly=PI)                      # and the inverse on the inputs designed for it
    assert _bad(c["inv_names"], d.download(), c["inv"]) == [], what
    d.free()
    eng.check()


FORMS = [(logn, "default", ()) for logn in SIZES]
FORMS += [(logn, "resident", (("ntt_resident", 1, 0),)) for logn in (13, 14)]
FORMS += [(logn, "fused", (("ntt_mode", 1, 0),)) for logn in (13, 14, 16, 17)]
FORMS += [(16, "packed", (("ntt_packed", 1, 0),))]


@pytest.mark.parametrize("logn,form,options", FORMS, ids=[f"{a}-{b}" for a, b, _ in FORMS])
def test_forward_and_inverse_on_designed_vectors(F, eng, O, logn, form, options):
    c = _case(O, logn)
    t = eng.tables(logn, c["qs"])
    assert t.paths == [0, 0] and t.psi == [L.psi for L in c["limbs"]]
    try:
        for name, on, _ in options:
            eng.set_option(name, on)
        _transforms(eng, t, c, (logn, form))
    finally:
        for name, _, off in options:
            eng.set_option(name, off)


def _some(c, logn):
    """the ladders, pulses at the first, second, middle and last stage, all q - 1 and q/2"""
    keep = {f"{k}pulse{t}" for k in "if" for t in (0, 1, logn // 2, logn - 1)} | {"all_qm1", "half"}
    return [p for p, n in enumerate(c["names"]) if n.startswith("ladder") or n in keep]


@pytest.mark.parametrize("logn", SIZES)
def test_polymul_on_designed_vectors(F, eng, O, logn):
    """the fused product: its middle launch runs the row passes lazily on both sides of the pointwise product, and its inverse
    enters from |x| < 0.6 q"""
    c = _case(O, logn)
    t = eng.tables(logn, c["qs"])
    idx = _some(c, logn)
    a = np.ascontiguousarray(c["data"][idx])
    rng = np.random.default_rng(logn)
    r = np.stack([np.stack([rng.integers(0, q, 1 << logn, dtype=np.uint64) for q in c["qs"]]) for _ in idx])
    for b in (a, r):
        da, db = eng.upload(a), eng.upload(b)
        t.polymul(da, da, db, n_poly=len(idx))
        got = da.download()
        for i, p in enumerate(idx):
            for l, L in enumerate(c["limbs"]):
                assert (got[i, l] == O.polymul_ntt(a[i, l], b[i, l], L.psi, L.q)).all(), (c["names"][p], l, b is a)
        da.free(), db.free()
    eng.check()


@pytest.mark.parametrize("n1,n2", [(16, 32), (256, 256)])
@pytest.mark.parametrize("bits", [50, 30])
def test_fourstep_on_ladders_and_pulses(F, eng, O, n1, n2, bits):
    """the natural-order transform (the inverse-structured network with a gathering first launch) on the vectors designed for ITS
    table (helpers/gs_worst_case.py: a pulse for every stage of the network, the constant and alternating patterns on its pair
    structure, spikes, words next to q), plain and checked: same words, every flag present and zero.  The negacyclic ladders and
    pulses this test once borrowed are solved through other tables and steer nothing here; its name is kept.  The oracle's
    four_step_ntt is the length-N transform with the root g^((q-1)/N); that is checked on the first vector, and the rest are compared
    with the oracle's O(N log N) form of the same sum and with the images the designed vectors come with (the cyclic transform)."""
    N = n1 * n2
    logn = N.bit_length() - 1
    L = G.GsLimb(logn, bits)
    q = L.q
    g = next(x for x in range(2, 1000) if pow(x, (q - 1) // 2, q) == q - 1)
    assert g == L.g
    fam = G.families(L)
    idx = list(range(len(fam)))
    assert len(idx) >= 2 * logn + 2
    x = np.stack([v for _, v, *_ in fam])
    w = pow(g, (q - 1) // N, q)
    want = np.stack([O.ntt_nthroot(v, w, q) for v in x])
    assert (want[0] == O.four_step_ntt(x[0], n1, n2, q, g)).all()
    assert (want == np.stack([L.oracle(v) for v in x])).all()
    fs = F.FourStep(eng, n1, n2, q, g)
    src, dst = eng.upload(x), eng.alloc(x.size)
    fs.ntt(src, dst, len(idx))
    assert (dst.download().reshape(x.shape) == want).all()
    dst2 = eng.alloc(x.size)
    flags = fs.ntt_checked(src, dst2, len(idx))
    assert (dst2.download().reshape(x.shape) == want).all()
    assert flags.shape == (len(idx),) and not flags.any()
    eng.check()


@pytest.mark.parametrize("logn", SIZES)
def test_checked_transforms_on_ladders_and_pulses(F, eng, O, logn):
    c = _case(O, logn)
    t = eng.tables(logn, c["qs"])
    ab = F.Abft(eng, t)
    idx = [p for p, n in enumerate(c["names"]) if "ladder" in n or "pulse" in n]
    data, fwd = np.ascontiguousarray(c["data"][idx]), c["fwd"][idx]
    d = eng.upload(data)
    flags = ab.forward_checked(d, n_poly=len(idx))
    assert flags.size == 2 * len(idx) and not flags.any()
    assert (d.download() == fwd).all()
    flags = ab.inverse_checked(d, n_poly=len(idx))
    assert flags.size == 2 * len(idx) and not flags.any()
    assert (d.download() == data).all()
    eng.check()


def test_integer_path_on_soak_patterns(F, eng, O):
    """parity on the soak patterns: Harvey's [0, 4q) has no fold schedule to break.  What it has is comparisons, x >= 2q and x >= q,
    which these patterns and random words never bring to equality: tests/test_gpu_integer_path_edges.py runs the integer path on
    inputs whose results vanish (tests/helpers/harvey_cases.py), where they meet it all the time."""
    for logn in (9, 13, 16):
        N = 1 << logn
        assert Q61 % (2 * N) == 1
        L = W.Limb.__new__(W.Limb)
        L.logn, L.N, L.q = logn, N, Q61
        rp = O.root_powers(Q61, logn)
        pats = W.soak_patterns(L)
        data = np.stack([v for _, v, *_ in pats])[:, None, :]
        t = eng.tables(logn, [Q61])
        assert t.paths == [1]
        d = eng.upload(data)
        t.forward(d, n_poly=len(pats))
        fwd = d.download()
        for p, (name, v, *_) in enumerate(pats):
            assert (fwd[p, 0] == O.nwt_forward(v, Q61, rp)).all(), (logn, name)
        t.inverse(d, n_poly=len(pats))
        assert (d.download() == data).all()
    eng.check()
