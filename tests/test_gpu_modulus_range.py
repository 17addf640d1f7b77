"""The transforms, the product and the pointwise calls on moduli between the three points the rest of the suite uses (the largest
30-, 50- and 61-bit primes).  One table set of four limbs per size:

  q_min(N)   the smallest prime that is 1 mod 2N (q - 1 a small multiple of 2N: indices, weights and scalars are not small beside q)
  q20        the largest prime of the 20-bit class that is 1 mod 2N and is not q_min(N); of the next class that holds one otherwise
  q50-       the last prime below 2^50 that is 1 mod 2N: the FP64 path's largest modulus
  q50+       the first one above 2^50: the integer path's smallest

The reference is tests/helpers/number_theory.py: its primes and minimal roots everywhere, its schoolbook sums at 2^4; above that
size the oracle's transforms run on the reference's roots (tests/test_host_math_range.py pins the oracle to the schoolbook sums at
2^4 and 2^6).  Every comparison is ==.

Sizes: 2^4 (all register steps in one launch), 2^10 (single launch), 2^13 (two launches), 2^16 (two-step rows).  Two polynomials
per call."""
import ctypes as C

import numpy as np
import pytest

from helpers import ntt_worst_case as W
from helpers import number_theory as NT

pytestmark = pytest.mark.gpu

SIZES = [4, 10, 13, 16]
ERR_INVALID, ERR_UNSUPPORTED = 1, 3
TOP = 2**64 - 1
U = np.uint64


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
def O():
    from oracle import cport
    return cport


def moduli(logn):
    N = 1 << logn
    q_min = NT.smallest_prime(N)
    q20 = next(p for bits in range(20, 40) for p in NT.primes_in_class(N, bits)[::-1] if p != q_min)
    return [q_min, q20, NT.last_prime_below(1 << 50, N), NT.first_prime_above(1 << 50, N)]


def _limb(O, logn, q, psi):
    """helpers/ntt_worst_case.py's Limb for a given prime (its own constructor takes the largest prime of a bit size)"""
    lm = W.Limb.__new__(W.Limb)
    lm.logn, lm.N, lm.bits, lm.q, lm.psi = logn, 1 << logn, q.bit_length(), q, psi
    lm.rp = O.root_powers(q, logn, psi)
    lm.rp_inv = O.root_powers(q, logn, pow(psi, -1, q))
    lm.half = (q + 1) // 2
    return lm


def _base_inputs(q, N, rng):
    """[(name, words)]: the inputs every limb takes; ``planted`` holds words outside [0, q), which every call reduces on load"""
    alt = np.where(np.arange(N) % 2 == 0, (q - 1) // 2, (q + 1) // 2).astype(U)
    first, last = np.zeros(N, dtype=U), np.zeros(N, dtype=U)
    first[0] = last[N - 1] = q - 1
    planted = rng.integers(0, q, N, dtype=U)
    for at, w in zip((0, 1, N // 2, N - 2, N - 1), (q, 2 * q - 1, 2**53 + 1, (2**64 // q) * q - 1, TOP)):
        planted[at] = w
    return [("random", rng.integers(0, q, N, dtype=U)), ("all_qm1", np.full(N, q - 1, dtype=U)), ("halves", alt), ("first", first), ("last", last),
            ("planted", planted)]


def _product(O, a, b, q, psi):
    if a.size <= NT.SCHOOLBOOK_MAX:
        return np.array(NT.negacyclic_product([int(v) for v in a], [int(v) for v in b], q), dtype=U)
    return O.polymul_ntt(a, b, psi, q)


_CASES = {}


def _case(O, logn):
    """The table set's reference and inputs with their images: computed once per size, shared, never modified.  data[p][l] is
    polynomial p's limb l as the calls receive it, canon the same words modulo q_l.  The first six polynomials are the base inputs
    for every limb; the rest carry a ladder or a pulse on the two limbs around 2^50 and random words on the other two."""
    if logn not in _CASES:
        N = 1 << logn
        qs = moduli(logn)
        psi = [NT.min_primitive_root(q, 2 * N) for q in qs]
        rp = np.array([NT.root_powers(q, logn, s)[0] for q, s in zip(qs, psi)], dtype=U)
        rng = np.random.default_rng(logn)
        cols, names = [], []
        for l, q in enumerate(qs):
            col = _base_inputs(q, N, rng)
            n_base = len(col)
            if l >= 2:
                lm = _limb(O, logn, q, psi[l])
                assert (lm.rp == rp[l]).all()
                for s0, K, canonical in W.forward_stretches(logn):
                    col.append((f"ladder{s0}+{K}", W.forward_ladder(lm, s0, K, canonical)[0]))
                for t in range(logn):
                    col.append((f"ipulse{t}", W.inverse_pulse(lm, t)[0]))
                    col.append((f"fpulse{t}", W.forward_pulse(lm, t)[0]))
            cols.append([v for _, v in col])
            names = [n for n, _ in col]
        for l in (0, 1):
            cols[l] += [rng.integers(0, qs[l], N, dtype=U) for _ in range(len(names) - n_base)]
        data = np.stack([np.stack([cols[l][p] for l in range(4)]) for p in range(len(names))])
        canon = data % np.array(qs, dtype=U)[None, :, None]
        P = len(names)
        if N <= NT.SCHOOLBOOK_MAX:
            fwd, inv = np.empty_like(canon), np.empty_like(canon)
            for p in range(P):
                for l, q in enumerate(qs):
                    x = [int(v) for v in canon[p, l]]
                    fwd[p, l] = NT.negacyclic_forward(x, q, psi[l])
                    inv[p, l] = NT.negacyclic_inverse(x, q, psi[l])
        else:                                          # the same two oracle calls on all rows at once
            fwd = O.nwt_forward_batch(canon.reshape(4 * P, N), np.tile(np.array(qs, dtype=U), P), np.tile(rp, (P, 1))).reshape(canon.shape)
            inv = O.nwt_inverse_batch(canon.reshape(4 * P, N), np.tile(np.array(qs, dtype=U), P), np.tile(rp, (P, 1))).reshape(canon.shape)
        for a in (data, canon, fwd, inv, rp):
            a.setflags(write=False)
        _CASES[logn] = dict(N=N, qs=qs, psi=psi, rp=rp, names=names, n_base=n_base, data=data, canon=canon, fwd=fwd, inv=inv)
    return _CASES[logn]


def _pairs(n):
    """two polynomials per call: (0, 1), (2, 3), ... and the last two once more when n is odd"""
    return [(p, p + 2) for p in range(0, n - 1, 2)] + ([(n - 2, n)] if n % 2 else [])


def _bad(names, got, want):
    return [(names[p], l) for p in range(got.shape[0]) for l in range(got.shape[1]) if not (got[p, l] == want[p, l]).all()]


def _transforms(eng, t, c, limbs, what):
    lo, hi = limbs
    for p0, p1 in _pairs(len(c["names"])):
        names = c["names"][p0:p1]
        data = np.ascontiguousarray(c["data"][p0:p1, lo:hi])
        d = eng.upload(data)
        t.forward(d, n_poly=2)
        assert _bad(names, d.download(), c["fwd"][p0:p1, lo:hi]) == [], what
        t.inverse(d, n_poly=2)                       # the round trip gives the input's residues back
        assert _bad(names, d.download(), c["canon"][p0:p1, lo:hi]) == [], what
        d.free()
        d = eng.upload(data)
        t.inverse(d, n_poly=2)
        assert _bad(names, d.download(), c["inv"][p0:p1, lo:hi]) == [], what
        d.free()
    eng.check()


def _products(eng, O, t, c, limbs, polys, what):
    """polynomial p times polynomial p + 1 (cyclically among ``polys``), both ways round"""
    lo, hi = limbs
    mate = {p: polys[(i + 1) % len(polys)] for i, p in enumerate(polys)}
    for i0, i1 in _pairs(len(polys)):
        ps = polys[i0:i1]
        a = np.ascontiguousarray(c["data"][ps][:, lo:hi])
        b = np.ascontiguousarray(c["data"][[mate[p] for p in ps]][:, lo:hi])
        want = np.stack([np.stack([_product(O, c["canon"][p, l], c["canon"][mate[p], l], c["qs"][l], c["psi"][l]) for l in range(lo, hi)]) for p in ps])
        for x, y in ((a, b), (b, a)):
            dx, dy, dz = eng.upload(x), eng.upload(y), eng.alloc(x.size)
            dz.shape = x.shape
            t.polymul(dz, dx, dy, n_poly=2)
            assert _bad([c["names"][p] for p in ps], dz.download(), want) == [], what
            dx.free(), dy.free(), dz.free()
    eng.check()


FORMS = [(logn, "default", ()) for logn in SIZES]
FORMS += [(logn, "fused", (("ntt_mode", 1, 0),)) for logn in (13, 16)]
FORMS += [(13, "resident", (("ntt_resident", 1, 0),))]


@pytest.mark.parametrize("logn,form,options", FORMS, ids=[f"{a}-{b}" for a, b, _ in FORMS])
def test_forward_inverse_and_round_trip(F, eng, O, logn, form, options):
    c = _case(O, logn)
    t = eng.tables(logn, c["qs"])
    assert t.paths == [0, 0, 0, 1] and t.psi == c["psi"]
    try:
        for name, on, _ in options:
            eng.set_option(name, on)
        _transforms(eng, t, c, (0, 4), (logn, form))
    finally:
        for name, _, off in options:
            eng.set_option(name, off)


@pytest.mark.parametrize("logn,form,options", FORMS, ids=[f"{a}-{b}" for a, b, _ in FORMS])
def test_polymul(F, eng, O, logn, form, options):
    """the base inputs and the ladders"""
    c = _case(O, logn)
    t = eng.tables(logn, c["qs"])
    polys = [p for p, n in enumerate(c["names"]) if p < c["n_base"] or n.startswith("ladder")]
    try:
        for name, on, _ in options:
            eng.set_option(name, on)
        _products(eng, O, t, c, (0, 4), polys, (logn, form))
    finally:
        for name, _, off in options:
            eng.set_option(name, off)


def _mulmod(O, a, b, q):
    """a b mod q on [rows][N] residues, q = [rows][1]: Python integers up to 2^10, the oracle's product above"""
    if a.shape[-1] <= 1 << 10:
        return (a.astype(object) * b.astype(object) % q.astype(object)).astype(U)
    return O.modmul_batch(a, b, q.ravel())


@pytest.mark.parametrize("logn", SIZES)
def test_pointwise_calls(F, eng, L, O, logn):
    """modmul, modmul_acc, modadd, modsub and scalar_affine with the scalars q - 1 and 2^64 - 1: the base inputs in pairs against the
    next pair, the planted out-of-range words in every operand position, the accumulator's old words included"""
    c = _case(O, logn)
    t, N, qs = eng.tables(logn, c["qs"]), c["N"], c["qs"]
    q = np.array(qs * 2, dtype=U).reshape(-1, 1)
    rows = lambda x: x.reshape(8, N)
    nb = c["n_base"]
    for p0 in range(0, nb, 2):
        sel = lambda k: [(p0 + k) % nb, (p0 + k + 1) % nb]
        a, b, o = (np.ascontiguousarray(c["data"][sel(k)]) for k in (0, 2, 4))
        ra, rb, ro = (rows(c["canon"][sel(k)]) for k in (0, 2, 4))
        da, db = eng.upload(a), eng.upload(b)

        def run(call, start=None):
            dc = eng.upload(np.full_like(a, 0x5E5E5E5E5E5E5E5E) if start is None else start)
            assert call(dc) in (0, None)
            got = rows(dc.download())
            dc.free()
            return got

        prod = _mulmod(O, ra, rb, q)
        assert (run(lambda dc: t.modmul(dc, da, db, n_poly=2)) == prod).all(), (logn, p0)
        assert (run(lambda dc: t.modmul(dc, da, db, n_poly=2, acc=True), start=o) == (ro + prod) % q).all(), (logn, p0)
        assert (run(lambda dc: L.fhe_modadd(eng._h, dc.ptr, da.ptr, db.ptr, t._h, 2, 4, 0, None)) == (ra + rb) % q).all(), (logn, p0)
        assert (run(lambda dc: L.fhe_modsub(eng._h, dc.ptr, da.ptr, db.ptr, t._h, 2, 4, 0, None)) == (ra + q - rb) % q).all(), (logn, p0)
        for mul, add in (([x - 1 for x in qs], [TOP] * 4), ([TOP] * 4, [x - 1 for x in qs])):
            m, s = ((C.c_uint64 * 4)(*v) for v in (mul, add))
            rm, rs = (np.array([v % x for v, x in zip(w, qs)] * 2, dtype=U).reshape(-1, 1) for w in (mul, add))
            want = (_mulmod(O, ra, np.broadcast_to(rm, ra.shape).copy(), q) + rs) % q
            assert (run(lambda dc: L.fhe_scalar_affine(eng._h, dc.ptr, da.ptr, m, s, t._h, 2, 4, 0, None)) == want).all(), (logn, p0, mul[0])
        da.free(), db.free()
    eng.check()


@pytest.mark.parametrize("logn", SIZES)
def test_automorphism(F, eng, O, logn):
    """x -> x^3 and x -> x^(2N-1): dst[(i k) mod N] = +-src[i], and the sign flip is q - v with v up to q - 1 for the tiny moduli"""
    c = _case(O, logn)
    t, N = eng.tables(logn, c["qs"]), c["N"]
    q = np.array(c["qs"], dtype=U).reshape(1, 4, 1)
    i = np.arange(N, dtype=np.int64)
    for k in (3, 2 * N - 1):
        j = i * k % (2 * N)
        for p0 in range(0, c["n_base"], 2):
            src = eng.upload(np.ascontiguousarray(c["data"][p0:p0 + 2]))
            dst = F.automorphism(eng, t, src, k, n_poly=2)
            v = c["canon"][p0:p0 + 2]
            want = np.empty_like(v)
            want[:, :, j % N] = np.where(j >= N, (q - v) % q, v)
            assert (dst.download() == want).all(), (logn, k, p0)
            src.free(), dst.free()
    eng.check()


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("logn", SIZES)
def test_forced_paths_on_the_small_moduli(F, eng, O, logn, path):
    """q_min(N) and the 20-bit prime through tables built from the reference's root powers, on the FP64 path and on the integer
    path: both take a modulus however small"""
    c = _case(O, logn)
    t = eng.tables_from_roots(logn, c["qs"][:2], c["rp"][:2], force_path=path)
    assert t.paths == [path, path] and t.psi == c["psi"][:2]
    _transforms(eng, t, c, (0, 2), (logn, path))
    _products(eng, O, t, c, (0, 2), list(range(c["n_base"])), (logn, path))


def test_statuses(F, eng, L):
    logn, N = 10, 1 << 10
    made = []

    def create(q):
        h = C.c_void_p()
        rc = L.fhe_ntt_tables_create(eng._h, logn, (C.c_uint64 * 1)(q), 1, C.byref(h))
        if rc == 0:
            made.append(h)
        return rc

    q62 = NT.primes_in_class(N, 62, 1)[0]
    assert q62 >> 61 == 1 and q62 % (2 * N) == 1
    assert create(q62) == ERR_UNSUPPORTED
    assert create(NT.first_prime_above(1 << 61, N)) == ERR_UNSUPPORTED
    q61 = NT.last_prime_below(1 << 61, N)
    assert create(q61) == 0
    paths, psi = (C.c_int * 1)(), (C.c_uint64 * 1)()
    assert L.fhe_ntt_tables_info(made[0], None, None, paths, psi) == 0
    assert list(paths) == [1] and int(psi[0]) == NT.min_primitive_root(q61, 2 * N)
    for q in ((1 << 50) - 1, 1 << 50, 12290, 12289 * 40961, 2):          # composite (the fourth of them 1 mod 2N), even, no 2N-th root
        assert create(q) == ERR_INVALID, q
    for q in (0, 1):
        assert create(q) == ERR_UNSUPPORTED, q
    assert L.fhe_last_error()
    for h in made:
        L.fhe_ntt_tables_destroy(h)


def test_engine_reports_no_error(eng):
    eng.check()
