"""Seals carried through the modular add and subtract, and the sealed rotate-and-sum, on the GPU.

Primitive: N = 2^5 (fewer words than lanes), 2^13 (exactly one chunk per row), 2^14 (the smallest row whose weights cross a chunk
boundary) on a table set of 50- and 61-bit primes; add and subtract, with and without locators, in place and out of place.  The
words are held against fhe_modadd / fhe_modsub and the carried seals against fhe_seal / fhe_seal_locator of the result (and against
Python integers), on rows designed for the wrap count: all q - 1, all zero, sums of exactly q - 1 and q, a = b, 0 - (q - 1).

Composite: plan A of test_gpu_seal.py (2^10, L 4, K 2, dnum 2) without and with plain modulus 65537, three steps with the Galois
elements 3^(2^s) mod 2N, against the chain of unchecked fhe_rotate + fhe_modadd."""
import ctypes as C

import numpy as np
import pytest

from helpers.checked_plan import limb_bits
from helpers.sealed_case import PLANS, flip, plain_modulus, py_seals_and_locator, raised, sealed_plan

pytestmark = pytest.mark.gpu

INVALID = 1
SUM, RANGE = 1, 2
GARBAGE = 0x5A5A5A5A5A5A5A5A
GRID_CAP = 8192                 # TENSOR_SEAL_GRID_CAP of ntt_launch.hpp: workgroups of the job loop at most
SHAPES = [(1, 1, 0), (3, 2, 1), (1, 7, 0)]


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


@pytest.fixture(scope="module")
def tables(F, eng):
    made = {}

    def get(logn):
        if logn not in made:
            qs = F.create_moduli(1 << logn, limb_bits("mixed", 5, 2))      # 50 61 50 61 50 | 61 50
            made[logn] = (qs, eng.tables(logn, qs))
        return made[logn]
    return get


def unchecked(eng, t, a, b, sub, **kw):
    """fhe_modadd / fhe_modsub into a fresh buffer"""
    from fhe_reliability_gpu_amd._lib import check, lib
    c = eng.alloc(a.size)
    c.shape = a.shape
    f = lib.fhe_modsub if sub else lib.fhe_modadd
    check(f(eng._h, c.ptr, a.ptr, b.ptr, t._h, kw["n_poly"], kw["limbs"], kw["start"], None))
    return c


def clone(eng, d):
    c = eng.alloc(d.size)
    c.shape = d.shape
    c.copy_from(d)
    eng.sync()
    return c


def designed_rows(rng, q_of, N):
    """operand rows [rows][N]: random ones and the rows the wrap count has to get right, in turn"""
    a, b = [], []
    for r, q in enumerate(q_of):
        x = rng.integers(0, q, N, dtype=np.uint64)
        kind = r % 7
        if kind == 0:
            y = rng.integers(0, q, N, dtype=np.uint64)
        elif kind == 1:
            x, y = np.full(N, q - 1, dtype=np.uint64), np.full(N, q - 1, dtype=np.uint64)      # add: every word wraps
        elif kind == 2:
            x, y = np.zeros(N, dtype=np.uint64), np.zeros(N, dtype=np.uint64)
        elif kind == 3:
            y = (q - 1 - x.astype(object)).astype(np.uint64)                                   # add: q - 1, no wrap
        elif kind == 4:
            x = rng.integers(1, q, N, dtype=np.uint64)
            y = (q - x.astype(object)).astype(np.uint64)                                       # add: exactly q, wraps to 0
        elif kind == 5:
            y = x.copy()                                                                       # sub: a = b
        else:
            x, y = np.zeros(N, dtype=np.uint64), np.full(N, q - 1, dtype=np.uint64)            # sub: 0 - (q - 1)
        a.append(x)
        b.append(y)
    return np.stack(a), np.stack(b)


# ---------------------------------------------------------------------------------------------------------------- primitive
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("logn", [5, 13, 14])
def test_carried_add_and_sub_give_the_unchecked_words_and_the_seal_of_the_result(F, eng, tables, logn, shape):
    n_poly, limbs, start = shape
    N = 1 << logn
    qs, t = tables(logn)
    rows = n_poly * limbs
    q_of = [qs[start + r % limbs] for r in range(rows)]
    kw = dict(limbs=limbs, start=start, n_poly=n_poly)
    for seed, maker in ((1, designed_rows), (2, lambda rng, q_of, N: tuple(np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in q_of]) for _ in range(2)))):
        ha, hb = maker(np.random.default_rng(1000 * logn + 10 * rows + seed), q_of, N)
        da, db = eng.upload(ha), eng.upload(hb)
        sa, sb = t.seal(da, **kw), t.seal(db, **kw)
        la, lb = t.seal_locator(da, **kw), t.seal_locator(db, **kw)
        for sub in (False, True):
            want = unchecked(eng, t, da, db, sub, **kw)
            hw = want.download()
            q_col = np.array(q_of, dtype=object).reshape(-1, 1)
            assert (hw.astype(object) == ((ha.astype(object) - hb.astype(object)) % q_col if sub else (ha.astype(object) + hb.astype(object)) % q_col)).all()
            want_seal, want_loc = t.seal(want, **kw).download(), t.seal_locator(want, **kw).download()
            if seed == 1:      # the library's own seal of the result is the Python-integer one
                ps = py_seals_and_locator(hw)
                assert want_seal.tolist() == [r[:2] for r in ps] and want_loc.tolist() == [r[2] for r in ps]
            call = t.modsub_sealed if sub else t.modadd_sealed
            for loc in (False, True):
                # out of place
                dc = eng.upload(np.full(ha.shape, GARBAGE, dtype=np.uint64))
                res = call(dc, da, db, sa, sb, locators=(la, lb) if loc else None, **kw)
                assert (dc.download() == hw).all(), (sub, loc)
                assert not res[-1].any(), (sub, loc, res[-1])
                assert (res[0].download() == want_seal).all(), (sub, loc)
                if loc:
                    assert (res[1].download() == want_loc).all(), sub
                # in place: c = a, seal_c = seal_a, locator_c = locator_a
                xa, xs, xl = clone(eng, da), clone(eng, sa), clone(eng, la)
                res = call(xa, xa, db, xs, sb, seal_c=xs, locators=(xl, lb, xl) if loc else None, **kw)
                assert (xa.download() == hw).all() and not res[-1].any(), (sub, loc)
                assert (xs.download() == want_seal).all(), (sub, loc)
                if loc:
                    assert (xl.download() == want_loc).all(), sub
        # the operands are untouched
        assert (da.download() == ha).all() and (db.download() == hb).all()
    eng.check()


def test_a_word_flipped_at_rest_raises_its_row_and_the_row_stays_raised(F, eng, tables):
    logn, (n_poly, limbs, start) = 13, (3, 2, 1)
    N = 1 << logn
    qs, t = tables(logn)
    rows = n_poly * limbs
    q_of = [qs[start + r % limbs] for r in range(rows)]
    kw = dict(limbs=limbs, start=start, n_poly=n_poly)
    rng = np.random.default_rng(5)
    ha, hb, hd = (np.stack([rng.integers(16, q - 16, N, dtype=np.uint64) for q in q_of]) for _ in range(3))
    da, db, dd = eng.upload(ha), eng.upload(hb), eng.upload(hd)
    sa, sb, sd = t.seal(da, **kw), t.seal(db, **kw), t.seal(dd, **kw)
    target, j = 3, N // 2 + 7
    only = lambda f: [0] * target + [f] + [0] * (rows - target - 1)
    flip(eng, da, target * N + j, 3)                                   # after sealing
    dc = eng.alloc(rows * N)
    dc.shape = ha.shape
    sc, fl = t.modadd_sealed(dc, da, db, sa, sb, **kw)
    assert fl.tolist() == only(SUM)
    assert (dc.download() == unchecked(eng, t, da, db, False, **kw).download()).all()      # fhe_modadd on the corrupted operand
    assert t.seal_verify(dc, sc, **kw).tolist() == only(SUM)
    # every other row's carried seal is the seal of its words
    good = t.seal(dc, **kw).download()
    assert [r for r in range(rows) if sc.download()[r].tolist() != good[r].tolist()] == [target]
    # a further carried add, then a subtract: still raised, that row alone
    de = eng.alloc(rows * N)
    de.shape = ha.shape
    se, fl = t.modadd_sealed(de, dc, dd, sc, sd, **kw)
    assert fl.tolist() == only(SUM)
    sf, fl = t.modsub_sealed(de, de, db, se, sb, seal_c=se, **kw)
    assert fl.tolist() == only(SUM)
    # a word that was never canonical: the range bit, and the words are still fhe_modadd's
    flip(eng, da, target * N + j, 3)
    assert not t.modadd_sealed(dc, da, db, sa, sb, **kw)[1].any()
    flip(eng, db, 1 * N + 5, 63)
    sc, fl = t.modadd_sealed(dc, da, db, sa, sb, **kw)
    assert fl.tolist() == [0, SUM | RANGE] + [0] * (rows - 2)
    assert (dc.download() == unchecked(eng, t, da, db, False, **kw).download()).all()
    eng.check()


def test_the_job_loop_takes_a_second_trip(F, eng):
    """cap + 1 rows of two words: the last row is workgroup 0's second job, the one the combine's trailing barrier is for.  With
    locators, the widest partial"""
    logn, N = 1, 2
    n_poly = GRID_CAP + 1
    qs = F.create_moduli(N, [50])
    t, q = eng.tables(logn, qs), qs[0]
    kw = dict(limbs=1, start=0, n_poly=n_poly)
    rng = np.random.default_rng(37)
    ha, hb = (rng.integers(0, q, (n_poly, N), dtype=np.uint64) for _ in range(2))
    assert ha.nbytes < 1 << 20
    da, db = eng.upload(ha), eng.upload(hb)
    sa, sb, la, lb = t.seal(da, **kw), t.seal(db, **kw), t.seal_locator(da, **kw), t.seal_locator(db, **kw)
    probe = (0, GRID_CAP - 1, GRID_CAP)
    for sub in (False, True):
        call = t.modsub_sealed if sub else t.modadd_sealed
        hw = ((ha.astype(object) - hb.astype(object)) % q if sub else (ha.astype(object) + hb.astype(object)) % q).astype(np.uint64)
        dc = eng.upload(np.full(ha.shape, GARBAGE, dtype=np.uint64))
        sc, lc, fl = call(dc, da, db, sa, sb, locators=(la, lb), **kw)
        assert not fl.any()
        assert (dc.download() == hw).all()
        sums, locs = sc.download().reshape(n_poly, 2), lc.download()
        for r in probe:
            want = py_seals_and_locator(hw[r:r + 1])[0]
            assert sums[r].tolist() == want[:2] and int(locs[r]) == want[2], (sub, r)
        assert (sums == t.seal(dc, **kw).download().reshape(n_poly, 2)).all() and (locs == t.seal_locator(dc, **kw).download()).all()
        # a word changed at rest in the last row raises exactly that row
        host = ha.copy()
        host[GRID_CAP, 1] ^= np.uint64(1)
        fl = call(dc, eng.upload(host), db, sa, sb, locators=(la, lb), **kw)[-1]
        assert np.flatnonzero(fl).tolist() == [GRID_CAP] and int(fl[GRID_CAP]) == SUM, sub
    eng.check()


@pytest.mark.parametrize("sub,loc", [(False, False), (True, True)])
def test_each_hook_point_raises_what_it_must_in_its_row_alone(F, eng, tables, sub, loc):
    from fhe_reliability_gpu_amd._lib import check, lib
    logn, (n_poly, limbs, start) = 14, (3, 2, 1)
    N = 1 << logn
    qs, t = tables(logn)
    rows = n_poly * limbs
    q_of = [qs[start + r % limbs] for r in range(rows)]
    kw = dict(limbs=limbs, start=start, n_poly=n_poly)
    rng = np.random.default_rng(6)
    ha, hb = (np.stack([rng.integers(16, q - 16, N, dtype=np.uint64) for q in q_of]) for _ in range(2))
    da, db = eng.upload(ha), eng.upload(hb)
    sa, sb = t.seal(da, **kw), t.seal(db, **kw)
    locs = (t.seal_locator(da, **kw), t.seal_locator(db, **kw)) if loc else None
    call = t.modsub_sealed if sub else t.modadd_sealed
    hw = unchecked(eng, t, da, db, sub, **kw).download()
    want_seal = t.seal(eng.upload(hw), **kw).download()
    target = 4
    only = lambda f: [0] * target + [f] + [0] * (rows - target - 1)
    dc = eng.alloc(rows * N)
    dc.shape = ha.shape
    for coeff in (0, (1 << 13) - 1, (1 << 13) + 6, N - 1):      # first word, either side of the chunk boundary, last word
        for point in range(5):
            bit = 3
            check(lib.fhe_ctx_inject_fault_seal_carry(eng._h, 0, point, target, coeff, bit))
            res = call(dc, da, db, sa, sb, locators=locs, **kw)
            got = dc.download()
            where = (point, coeff)
            if point in (0, 1):
                x = [ha.copy(), hb.copy()]
                x[point][target, coeff] ^= np.uint64(1 << bit)
                q = q_of[target]
                w = (int(x[0][target, coeff]) - int(x[1][target, coeff])) % q if sub else (int(x[0][target, coeff]) + int(x[1][target, coeff])) % q
                assert res[-1].tolist() == only(SUM), where
                assert int(got[target, coeff]) == w and np.argwhere(got != hw).tolist() == [[target, coeff]], where
            elif point == 2:
                assert res[-1].tolist() == only(SUM), where
                assert np.argwhere(got != hw).tolist() == [[target, coeff]] and int(got[target, coeff]) == int(hw[target, coeff]) ^ (1 << bit), where
            elif point == 3:
                assert not res[-1].any(), where
                assert np.argwhere(got != hw).tolist() == [[target, coeff]] and int(got[target, coeff]) == int(hw[target, coeff]) ^ (1 << bit), where
                assert (res[0].download() == want_seal).all(), where
                assert t.seal_verify(dc, res[0], **kw).tolist() == only(SUM if int(got[target, coeff]) < q_of[target] else SUM | RANGE), where
            else:
                assert res[-1].tolist() == only(SUM) and (got == hw).all(), where
            # memory stayed clean and the hook was one shot: the same call again raises nothing
            assert (da.download() == ha).all() and (db.download() == hb).all()
            res = call(dc, da, db, sa, sb, locators=locs, **kw)
            assert not res[-1].any() and (dc.download() == hw).all() and (res[0].download() == want_seal).all(), where
    # call = 1: the hook waits for the second carry launch
    check(lib.fhe_ctx_inject_fault_seal_carry(eng._h, 1, 2, target, 9, 3))
    assert not call(dc, da, db, sa, sb, locators=locs, **kw)[-1].any()
    assert call(dc, da, db, sa, sb, locators=locs, **kw)[-1].tolist() == only(SUM)
    assert not call(dc, da, db, sa, sb, locators=locs, **kw)[-1].any()
    eng.check()


def test_argument_rules_return_their_status_with_nothing_launched(F, eng, tables):
    from fhe_reliability_gpu_amd._lib import check, lib
    qs, t = tables(13)
    N = 1 << 13
    rng = np.random.default_rng(1)
    ha, hb = (np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs[:2]]) for _ in range(2))
    da, db = eng.upload(ha), eng.upload(hb)
    sa, sb = t.seal(da, limbs=2), t.seal(db, limbs=2)
    la, lb = t.seal_locator(da, limbs=2), t.seal_locator(db, limbs=2)
    dc = eng.upload(np.full(2 * N + 2, GARBAGE, dtype=np.uint64))
    sc = eng.upload(np.full(4, GARBAGE, dtype=np.uint64))
    lc = eng.upload(np.full(2, GARBAGE, dtype=np.uint64))
    fl = eng.upload(np.full(2, GARBAGE, dtype=np.uint64))
    off = lambda d: C.c_void_p(d.ptr.value + 8)

    def untouched():
        return all((x.download() == GARBAGE).all() for x in (dc, sc, lc, fl))

    for f in (lib.fhe_modadd_sealed, lib.fhe_modsub_sealed):
        run = lambda c=dc.ptr, a=da.ptr, b=db.ptr, s_c=sc.ptr, s_a=sa.ptr, s_b=sb.ptr, l_c=None, l_a=None, l_b=None, limbs=2, start=0: f(
            eng._h, c, a, b, s_c, s_a, s_b, l_c, l_a, l_b, t._h, 1, limbs, start, fl.ptr, None)
        # misalignment of each buffer
        assert run(c=off(dc)) == INVALID and run(a=off(da)) == INVALID and run(b=off(db)) == INVALID
        # a null seal
        assert run(s_c=None) == INVALID and run(s_a=None) == INVALID and run(s_b=None) == INVALID
        assert b"seal" in lib.fhe_last_error()
        # partly given locators
        assert run(l_a=la.ptr, l_b=lb.ptr) == INVALID and run(l_c=lc.ptr) == INVALID and run(l_c=lc.ptr, l_a=la.ptr) == INVALID
        assert b"all three or none" in lib.fhe_last_error()
        # a window outside the table set
        assert run(limbs=2, start=len(qs) - 1) == INVALID
        # a hook row or word outside the call: refused, used up
        for row, coeff in ((2, 0), (0, N)):
            check(lib.fhe_ctx_inject_fault_seal_carry(eng._h, 0, 2, row, coeff, 3))
            assert run() == INVALID
        assert untouched()
        # nothing to do: FHE_OK, nothing touched
        assert f(eng._h, dc.ptr, da.ptr, db.ptr, sc.ptr, sa.ptr, sb.ptr, None, None, None, t._h, 0, 2, 0, fl.ptr, None) == 0
        assert f(eng._h, dc.ptr, da.ptr, db.ptr, sc.ptr, sa.ptr, sb.ptr, None, None, None, t._h, 1, 0, 0, fl.ptr, None) == 0
        assert untouched()
    # the setter: points 0 .. 4, bits 0 .. 63, a call number that is not negative; row < 0 clears
    bad = [(0, 5, 0, 0, 0), (0, 0, 0, 0, 64), (0, 0, 0, -1, 0), (-1, 0, 0, 0, 0), (0, -1, 0, 0, 0)]
    assert all(lib.fhe_ctx_inject_fault_seal_carry(eng._h, *x) == INVALID for x in bad)
    check(lib.fhe_ctx_inject_fault_seal_carry(eng._h, 0, 2, 1, 5, 0))
    check(lib.fhe_ctx_inject_fault_seal_carry(eng._h, 0, 0, -1, 0, 0))
    seal, flags = t.modadd_sealed(dc, da, db, sa, sb, limbs=2)
    assert not flags.any() and (seal.download() == t.seal(dc, limbs=2).download()).all()
    eng.check()


# ---------------------------------------------------------------------------------------------------------------- composite
GALOIS = [3, 9, 81]      # 3^(2^s) mod 2N, N = 2^10


class Case:
    """plan A, its detector, seeded accumulators and one Galois key per step on the device, and their seals"""

    def __init__(self, F, eng):
        self.logn, self.L, self.K, self.dnum, _ = PLANS["A"]
        self.N, self.M = 1 << self.logn, self.L + self.K
        self.qs, self.t, self.ks, self.ab = sealed_plan(F, eng, PLANS["A"])
        rng = np.random.default_rng(self.logn)
        self.c = [np.stack([rng.integers(16, q - 16, self.N, dtype=np.uint64) for q in self.qs[:self.L]]) for _ in range(2)]
        self.keys = [eng.upload(np.stack([rng.integers(0, q, self.N, dtype=np.uint64) for _ in range(2 * self.dnum) for q in self.qs])) for _ in GALOIS]
        self.d = [eng.upload(v) for v in self.c]
        self.seals = [self.t.seal(v, limbs=self.L) for v in self.d]
        self.key_seals = [self.ks.seal_key(k) for k in self.keys]
        assert all(pow(3, 1 << s, 2 * self.N) == g for s, g in enumerate(GALOIS))


@pytest.fixture(scope="module")
def case(F, eng):
    return Case(F, eng)


def run(c, d=None):
    return c.ks.rotate_sum_sealed(*(d or c.d), GALOIS, c.keys, c.ab, c.seals, key_seals=c.key_seals)


@pytest.mark.parametrize("tp", [0, 65537])
def test_clean_rotate_and_sum_gives_the_unchecked_chain_no_flag_and_the_final_seals(F, eng, case, tp):
    from fhe_reliability_gpu_amd._lib import check, lib
    c = case
    ks, L = c.ks, c.L
    with plain_modulus(ks, tp):
        lay, rl = ks.rotate_sum_sealed_layout(len(GALOIS)), ks.rotate_sealed_layout()
        assert lay["add"] == rl["total"] and lay["stride"] == rl["total"] + 2 * L and lay["total"] == len(GALOIS) * lay["stride"]
        o0, o1, so, steps = run(c)
        assert [raised(s) for s in steps] == [[]] * len(GALOIS)
        assert sorted(steps[0]) == ["add0", "add1", "c0", "c1", "checked", "key"]
        # the chain of unchecked calls
        w = [clone(eng, c.d[0]), clone(eng, c.d[1])]
        for g, key in zip(GALOIS, c.keys):
            r = ks.rotate(w[0], w[1], g, key)
            for h in range(2):
                check(lib.fhe_modadd(eng._h, w[h].ptr, w[h].ptr, r[h].ptr, c.t._h, 1, L, 0, None))
        assert (o0.download() == w[0].download()).all() and (o1.download() == w[1].download()).all()
        for h in range(2):
            assert (so[h].download() == c.t.seal(w[h], limbs=L).download()).all()
            assert so[h].download().tolist() == [r[:2] for r in py_seals_and_locator(w[h].download())]
        # the inputs and their seals are untouched
        assert all((dv.download() == v).all() for dv, v in zip(c.d, c.c))
    eng.check()


@pytest.mark.parametrize("tp", [0, 65537])
def test_faults_at_rest_and_in_the_adds_show_where_the_layout_says(F, eng, case, tp):
    from fhe_reliability_gpu_amd._lib import check, lib
    c = case
    ks, L, N = c.ks, c.L, c.N
    row, j = 2, N // 2 + 3
    only = lambda f: [bool(x) for x in f] == [r == row for r in range(L)]
    with plain_modulus(ks, tp):
        # a word of c0 flipped at rest before the call: step 0's input row, no row of the key
        d0 = clone(eng, c.d[0])
        flip(eng, d0, row * N + j, 3)
        steps = run(c, (d0, c.d[1]))[3]
        assert steps[0]["c0"].tolist() == [SUM if r == row else 0 for r in range(L)]
        assert not steps[0]["key"].any() and not steps[0]["c1"].any()
        # the carry hook after the digest of add 0 (step 0, c0): nothing in step 0, exactly that row of step 1's input block
        check(lib.fhe_ctx_inject_fault_seal_carry(eng._h, 0, 3, row, j, 0))
        steps = run(c)[3]
        assert raised(steps[0]) == []
        assert only(steps[1]["c0"]) and int(steps[1]["c0"][row]) & SUM and not steps[1]["c1"].any() and not steps[1]["key"].any()
        # the carry hook before the digest of add 2 (step 1, c0): that add row, the same row of step 2's input block, nothing before
        check(lib.fhe_ctx_inject_fault_seal_carry(eng._h, 2, 2, row, j, 0))
        steps = run(c)[3]
        assert raised(steps[0]) == []
        assert raised({k: v for k, v in steps[1].items() if k not in ("add0", "add1")}) == []
        assert steps[1]["add0"].tolist() == [SUM if r == row else 0 for r in range(L)] and not steps[1]["add1"].any()
        assert only(steps[2]["c0"]) and int(steps[2]["c0"][row]) & SUM and not steps[2]["c1"].any() and not steps[2]["key"].any()
        # one shot: clean again
        assert [raised(s) for s in run(c)[3]] == [[]] * len(GALOIS)
        # a hook row outside the composite's adds: refused with nothing launched
        check(lib.fhe_ctx_inject_fault_seal_carry(eng._h, 5, 2, L, 0, 0))
        with pytest.raises(F.FheError):
            run(c)
        assert [raised(s) for s in run(c)[3]] == [[]] * len(GALOIS)
    eng.check()
