"""The integer path (q >= 2^50: Harvey butterflies, lazy words in [0, 4q) / [0, 2q), one Barrett step for a product of lazy words) on
the inputs of tests/helpers/harvey_cases.py, where exact results vanish and every ``>=`` of modarith.hpp ArithU64 meets equality:
the transforms in every form, the negacyclic product with its result aliased to either factor, the checked and the sealed forms,
and the natural-order transform.  tests/test_harvey_cases.py shows on a model what each family is for and that random vectors
cannot stand in for them; tests/test_emu_harvey_cases.py counts the equalities on the kernels' own templates.

One table set per size: the two largest primes below 2^61, the smallest prime above 2^50 -- the three integer-path moduli -- and a
50-bit and a 30-bit limb, which carry the same families on the FP64 path (parity, and ArithF64::canonical's sign fix on +-0).
Every comparison is == against the oracle, and every output word is below its modulus."""
import numpy as np
import pytest

from helpers import harvey_cases as H
from helpers import ntt_worst_case as W
from helpers.sealed_case import py_seals

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


_CASES = {}


def case(logn):
    """the five limbs and their families, stacked [P][5][N] with the oracle's words beside them: built once per size, read-only"""
    if logn not in _CASES:
        qs = H.moduli(logn) + [W.prime_below(50, logn), W.prime_below(30, logn)]
        limbs = [H.Limb(logn, q) for q in qs]
        c = dict(qs=qs, limbs=limbs, Q=np.array(qs, dtype=np.uint64)[None, :, None])
        for key, inverse in (("fwd", False), ("inv", True)):
            fams = [H.transform_families(L, inverse, integer_path=k < 3) for k, L in enumerate(limbs)]
            c[key + "_names"] = [n for n, *_ in fams[0]]
            c[key + "_in"] = np.stack([np.stack([f[p][1] for f in fams]) for p in range(len(fams[0]))])
            c[key + "_out"] = np.stack([np.stack([f[p][2] for f in fams]) for p in range(len(fams[0]))])
        prods = [H.product_families(L) for L in limbs]
        c["prod_names"] = [n for n, *_ in prods[0]]
        for j, key in ((1, "a"), (2, "b"), (3, "c")):
            c[key] = np.stack([np.stack([f[p][j] for f in prods]) for p in range(len(prods[0]))])
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CASES[logn] = c
    return _CASES[logn]


def _tables(eng, c, logn):
    t = eng.tables(logn, c["qs"])
    assert t.paths == [1, 1, 1, 0, 0] and t.psi == [L.psi for L in c["limbs"]]
    return t


def _bad(names, got, want, Q):
    """[(family, limb)] whose words differ from the oracle's or are not below the modulus"""
    got = got.reshape(want.shape)
    return [(names[p], l) for p in range(want.shape[0]) for l in range(want.shape[1])
            if not ((got[p, l] == want[p, l]).all() and (got[p, l] < Q[0, l, 0]).all())]


DEFAULTS = {"ntt_resident": 0, "ntt_mode": 0, "tile_geo": 1, "ntt_chunk_mib": 96, "ntt_chunk_floor_mib": 192, "ntt_split": -1,
            "ntt_pingpong": -1, "ntt_stream": -1}
CUT = (("ntt_chunk_mib", 1), ("ntt_chunk_floor_mib", 0), ("ntt_split", 1), ("ntt_pingpong", 1), ("ntt_stream", 1))
FORMS = [(logn, "default", ()) for logn in (1, 3, 9, 12, 13, 14, 16)]
FORMS += [(logn, "resident", (("ntt_resident", 1),)) for logn in (13, 14)]
FORMS += [(logn, "fused", (("ntt_mode", 1),)) for logn in (13, 16)]
FORMS += [(16, "geo0", (("tile_geo", 0),)), (16, "cut", CUT)]


@pytest.mark.parametrize("logn,form,options", FORMS, ids=[f"{a}-{b}" for a, b, _ in FORMS])
def test_forward_and_inverse_batch(eng, logn, form, options):
    """forward and inverse on the families built for each, and the round trip; "cut": sub-batches of 1 MiB on alternating streams
    with the hand-off through the per-stream scratch, where lazy 64-bit words cross memory between launches and streams"""
    c = case(logn)
    t = _tables(eng, c, logn)
    try:
        for name, value in options:
            eng.set_option(name, value)
        for key in ("fwd", "inv"):
            names, P = c[key + "_names"], len(c[key + "_names"])
            run, back = (t.forward, t.inverse) if key == "fwd" else (t.inverse, t.forward)
            assert form != "cut" or c[key + "_in"].nbytes > (3 << 19)           # (past 1.5 sub-batches: the call is cut)
            d = eng.upload(c[key + "_in"])
            run(d, n_poly=P)
            assert _bad(names, d.download(), c[key + "_out"], c["Q"]) == [], (logn, form, key)
            back(d, n_poly=P)                                                   # the round trip gives the input's residues back
            assert _bad(names, d.download(), c[key + "_in"] % c["Q"], c["Q"]) == [], (logn, form, key)
            d.free()
        eng.check()
    finally:
        for name, _ in options:
            eng.set_option(name, DEFAULTS[name])


def test_limb_window_and_three_polynomials(eng):
    """start_idx = 1, three limbs (two integer-path, one FP64), three polynomials, at the first two-launch size"""
    logn, start, limbs, P = 13, 1, 3, 3
    c = case(logn)
    t = _tables(eng, c, logn)
    Q = c["Q"][:, start:start + limbs]
    for key, run in (("fwd", t.forward), ("inv", t.inverse)):
        pick = [c[key + "_names"].index(n) for n in ("zero", "lifted_slot_0", "odd")]
        d = eng.upload(np.ascontiguousarray(c[key + "_in"][pick][:, start:start + limbs]))
        run(d, limbs=limbs, start=start, n_poly=P)
        assert _bad([c[key + "_names"][p] for p in pick], d.download(), c[key + "_out"][pick][:, start:start + limbs], Q) == [], key
        d.free()
    eng.check()


@pytest.mark.parametrize("logn", [3, 12, 13, 16])
def test_polymul_with_the_result_aliased_to_either_factor(F, eng, logn):
    """disjoint spectra (every pointwise product a multiple of q, the result all zero), spectra that meet in one slot, and x^j
    against zeros at known places; polymul_checked on the same factors: the same words, no flag"""
    c = case(logn)
    t = _tables(eng, c, logn)
    ab = F.Abft(eng, t)
    P = len(c["prod_names"])
    for alias in ("a", "b", "checked"):
        da, db = eng.upload(c["a"]), eng.upload(c["b"])
        if alias == "checked":
            flags = ab.polymul_checked(da, da, db, n_poly=P)
            assert flags.shape == (5 * P, 3) and not flags.any(), logn
        else:
            t.polymul(da if alias == "a" else db, da, db, n_poly=P)
        got = (db if alias == "b" else da).download()
        assert _bad(c["prod_names"], got, c["c"], c["Q"]) == [], (logn, alias)
        da.free(), db.free()
    eng.check()


@pytest.mark.parametrize("logn", [3, 12, 13, 16])
def test_checked_transforms(F, eng, logn):
    c = case(logn)
    t = _tables(eng, c, logn)
    ab = F.Abft(eng, t)
    for key, run in (("fwd", ab.forward_checked), ("inv", ab.inverse_checked)):
        P = len(c[key + "_names"])
        d = eng.upload(c[key + "_in"])
        flags = run(d, n_poly=P)
        assert flags.size == 5 * P and not flags.any(), (logn, key)
        assert _bad(c[key + "_names"], d.download(), c[key + "_out"], c["Q"]) == [], (logn, key)
        d.free()
    eng.check()


def _unlifted(c, key):
    """the sealed calls hold every loaded word to its window, so a lifted word raises SEAL_RANGE by design: the families in range"""
    idx = [p for p, n in enumerate(c[key + "_names"]) if not n.startswith("lifted_")]
    return idx, np.ascontiguousarray(c[key + "_in"][idx]), c[key + "_out"][idx]


@pytest.mark.parametrize("logn", [12, 13])
def test_sealed_transforms(F, eng, logn):
    """ntt_sealed, intt_sealed and intt_sealed_out: the oracle's words, no flag, and the stored seal equal to the Python-integer
    seal of the ORACLE's words -- a word q or 2q in place of 0 would shift both of its sums"""
    c = case(logn)
    t = _tables(eng, c, logn)
    ab = F.Abft(eng, t)
    for key, calls in (("fwd", (t.ntt_sealed,)), ("inv", (t.intt_sealed_out, t.intt_sealed))):
        idx, x, want = _unlifted(c, key)
        names, P = [c[key + "_names"][p] for p in idx], len(idx)
        src = eng.upload(x)
        seal = t.seal(src, n_poly=P)
        assert seal.download().reshape(-1, 2).tolist() == py_seals(x)
        for call in calls:
            out = call(src, seal, ab, n_poly=P)
            dst, fl = out[0], out[-1]
            assert fl.shape == (2, 5 * P) and not fl.any(), (logn, key)
            assert _bad(names, dst.download(), want, c["Q"]) == [], (logn, key)
            if len(out) == 3:
                assert out[1].download().reshape(-1, 2).tolist() == py_seals(want), (logn, key)
    eng.check()


@pytest.mark.parametrize("logn", [12, 13])
def test_sealed_polymul(F, eng, logn):
    c = case(logn)
    t = _tables(eng, c, logn)
    ab = F.Abft(eng, t)
    P = len(c["prod_names"])
    for alias in ("a", "b"):
        da, db = eng.upload(c["a"]), eng.upload(c["b"])
        seal_a, seal_b = t.seal(da, n_poly=P), t.seal(db, n_poly=P)
        dc = da if alias == "a" else db
        seal_c, fl = ab.polymul_sealed(dc, da, db, seal_a, seal_b, n_poly=P)
        assert not fl["a"].any() and not fl["b"].any() and not fl["checked"].any(), (logn, alias)
        assert _bad(c["prod_names"], dc.download(), c["c"], c["Q"]) == [], (logn, alias)
        assert seal_c.download().reshape(-1, 2).tolist() == py_seals(c["c"]), (logn, alias)
        da.free(), db.free()
    eng.check()


# ------------------------------------------------------------------ natural order
def _cyclic(eng, x, logn, q, root, convention, inverse):
    from fhe_reliability_gpu_amd._lib import check, lib
    d, s = eng.upload(x), eng.alloc(x.size)
    check(lib.fhe_ntt_cyclic(eng._h, d.ptr, s.ptr, logn, x.shape[0], q, root, convention, inverse, None))
    out = d.download().reshape(x.shape)
    d.free(), s.free()
    return out


@pytest.mark.parametrize("logn,n1", [(4, 4), (5, 4), (12, 64), (13, 64)])
def test_natural_order_forms(F, eng, logn, n1):
    """fhe_ntt_cyclic forward and inverse under both root conventions, and the four-step batch, on vanishing and sparse spectra of
    the cyclic transform over the largest prime below 2^61: 2^4 takes the forward-network route, the rest the natural-order launches"""
    Cy = H.CyclicLimb(logn)
    q = np.uint64(Cy.q)
    eng.trace(True)
    try:
        for inverse in (0, 1):
            fam = H.natural_families(Cy, bool(inverse))
            x, want = np.stack([v for _, v, *_ in fam]), np.stack([w for _, _, w, _ in fam])
            for convention, root in ((0, Cy.g), (1, Cy.w)):
                got = _cyclic(eng, x, logn, Cy.q, root, convention, inverse)
                bad = [n for (n, *_), g, w in zip(fam, got, want) if not ((g == w).all() and (g < q).all())]
                assert bad == [], (logn, inverse, convention)
            if not inverse:
                fs = F.FourStep(eng, n1, (1 << logn) // n1, Cy.q, Cy.g)
                src, dst = eng.upload(x), eng.alloc(x.size)
                fs.ntt(src, dst, len(fam))
                got = dst.download().reshape(x.shape)
                assert [n for (n, *_), g, w in zip(fam, got, want) if not ((g == w).all() and (g < q).all())] == [], logn
                fs.close()
    finally:
        eng.trace(False)
    text = eng.trace_text()
    route, other = ("NTT_CYCLIC_FORWARD_NETWORK", "NTT_CYCLIC_NATURAL_ORDER") if logn < 5 else ("NTT_CYCLIC_NATURAL_ORDER", "NTT_CYCLIC_FORWARD_NETWORK")
    assert text.count(route) >= 4 and other not in text, text
    eng.check()
