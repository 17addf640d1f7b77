"""Seals of rows at rest and the sealed multiply / rotation on the GPU.  Seals are held against Python integers computed here from
the host arrays, never against fhe_seal itself.

Primitives: N = 2^5 (below one workgroup), 2^13 (one chunk per row), 2^16 (eight chunks per row) on mixed 50 / 61-bit tables; a
flip of one word in memory raises exactly its row, the multi-bit change a fold modulo 2^32 - 1 cannot see included.

Composites: plans A (2^10, L 4, K 2, dnum 2) and B (2^13, L 3, K 1, dnum 3, a 61-bit prime among 50-bit ones) of
test_gpu_bgv_checked.py, each without and with plain modulus 65537.  One flipped bit in an operand or in the key raises exactly its
row of the seal blocks, while the checked call alone computes on the flipped operand and raises nothing: the gap and its closure."""
import ctypes as C

import numpy as np
import pytest

from helpers.checked_plan import limb_bits
from helpers.sealed_case import SealedCase, case_cache, flip, plain_modulus, plans, py_seals, raised, safe_coeff, same

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
SUM, RANGE = 1, 2
GARBAGE = 0x5A5A5A5A5A5A5A5A
PLANS = plans("AB")
SHAPES = [(1, 1, 0), (3, 2, 1), (1, 7, 0)]


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


# ---------------------------------------------------------------------------------------------------------------- primitives
@pytest.fixture(scope="module")
def tables(F, eng):
    made = {}

    def get(logn):
        if logn not in made:
            qs = F.create_moduli(1 << logn, limb_bits("mixed", 5, 2))      # 50 61 50 61 50 | 61 50
            made[logn] = (qs, eng.tables(logn, qs))
        return made[logn]
    return get


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("logn", [5, 13, 16])
def test_seal_and_verify(F, eng, tables, logn, shape):
    from fhe_reliability_gpu_amd._lib import check, lib
    n_poly, limbs, start = shape
    N = 1 << logn
    qs, t = tables(logn)
    rows = n_poly * limbs
    q_of = [qs[start + r % limbs] for r in range(rows)]
    rng = np.random.default_rng(100 * logn + rows)
    x = np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in q_of])
    x[-1] = q_of[-1] - 1                                     # a row of all q - 1
    # the words the flips below hit: first and last of a row, either side of a chunk boundary (of the row's middle at the sizes of
    # one chunk) -- small values, so that a flipped bit 3 stays below q
    mid = 1 << 13 if logn > 13 else N // 2
    spots = [0, mid - 1, mid, N - 1]
    target = rows // 2
    x[target, spots] = [12345, 2**40 + 5, 777, 99]
    d = eng.upload(x)
    want = py_seals(x)
    kw = dict(limbs=limbs, start=start, n_poly=n_poly)
    s = t.seal(d, **kw)
    assert s.download().tolist() == want
    # reruns into other buffers: identical seals, bit for bit (the combine is integer arithmetic modulo p)
    assert all(t.seal(d, **kw).download().tobytes() == s.download().tobytes() for _ in range(3))
    assert not t.seal_verify(d, s, **kw).any()
    only = lambda f: [0] * target + [f] + [0] * (rows - target - 1)
    # one flipped bit in memory, at each spot: exactly that row, the sum bit alone
    for j in spots:
        flip(eng, d, target * N + j, 3)
        assert t.seal_verify(d, s, **kw).tolist() == only(SUM), j
        flip(eng, d, target * N + j, 3)
    assert (d.download() == x).all() and not t.seal_verify(d, s, **kw).any()
    # +2^8 - 2^40 inside one word, written from the host: invisible modulo 2^32 - 1
    y = x.copy()
    y[target, mid - 1] = 5 + 2**8
    assert ((int(y[target, mid - 1]) - int(x[target, mid - 1])) % (2**32 - 1)) == 0
    assert t.seal_verify(eng.upload(y), s, **kw).tolist() == only(SUM)
    # a word set to q: the window (and the sum: q - x is not 0 modulo p)
    y = x.copy()
    y[target, N - 1] = q_of[target]
    assert t.seal_verify(eng.upload(y), s, **kw).tolist() == only(SUM | RANGE)
    # the hook flips the loaded word in the register: its row is raised, memory stays clean, the next call is clean
    for j in spots:
        check(lib.fhe_ctx_inject_fault_seal(eng._h, target, j, 3))
        assert t.seal_verify(d, s, **kw).tolist() == only(SUM), j
        assert not t.seal_verify(d, s, **kw).any()
    check(lib.fhe_ctx_inject_fault_seal(eng._h, target, 0, 62))
    assert t.seal_verify(d, s, **kw).tolist() == only(SUM | RANGE)
    assert (d.download() == x).all()
    # on fhe_seal the hook seals the flipped word: that row's seal differs, and the clean data fail it
    check(lib.fhe_ctx_inject_fault_seal(eng._h, target, N - 1, 3))
    bad = t.seal(d, **kw)
    got = bad.download().tolist()
    assert [r for r in range(rows) if got[r] != want[r]] == [target]
    assert t.seal_verify(d, bad, **kw).tolist() == only(SUM)
    assert t.seal(d, **kw).download().tolist() == want
    eng.check()


def test_seal_argument_rules(F, eng, tables):
    from fhe_reliability_gpu_amd._lib import check, lib
    qs, t = tables(13)
    N = 1 << 13
    x = np.stack([np.random.default_rng(1).integers(0, q, N, dtype=np.uint64) for q in qs[:2]])
    d = eng.upload(x)
    s = eng.upload(np.full(4, GARBAGE, dtype=np.uint64))
    fl = eng.upload(np.full(2, GARBAGE, dtype=np.uint64))
    # nothing to do: FHE_OK, nothing touched
    for n_poly, limbs in ((0, 2), (1, 0)):
        check(lib.fhe_seal(eng._h, s.ptr, d.ptr, t._h, n_poly, limbs, 0, None))
        check(lib.fhe_seal_verify(eng._h, d.ptr, s.ptr, t._h, n_poly, limbs, 0, fl.ptr, None))
    assert (s.download() == GARBAGE).all() and (fl.download() == GARBAGE).all()
    # a window outside the table set, a misaligned buffer
    assert lib.fhe_seal(eng._h, s.ptr, d.ptr, t._h, 1, 2, len(qs) - 1, None) == INVALID
    assert lib.fhe_seal_verify(eng._h, d.ptr, s.ptr, t._h, 1, len(qs) + 1, 0, fl.ptr, None) == INVALID
    assert lib.fhe_seal(eng._h, s.ptr, C.c_void_p(d.ptr.value + 8), t._h, 1, 1, 0, None) == INVALID
    # a hook outside the call: refused, nothing launched, used up
    for row, coeff in ((2, 0), (0, N)):
        check(lib.fhe_ctx_inject_fault_seal(eng._h, row, coeff, 0))
        assert lib.fhe_seal_verify(eng._h, d.ptr, s.ptr, t._h, 1, 2, 0, fl.ptr, None) == INVALID
        assert (fl.download() == GARBAGE).all()
    assert lib.fhe_ctx_inject_fault_seal(eng._h, 0, 0, 64) == INVALID and lib.fhe_ctx_inject_fault_seal(eng._h, 0, -1, 0) == INVALID
    good = t.seal(d, limbs=2)
    assert good.download().tolist() == py_seals(x) and not t.seal_verify(d, good, limbs=2).any()
    check(lib.fhe_ctx_inject_fault_seal(eng._h, 1, 5, 0))
    check(lib.fhe_ctx_inject_fault_seal(eng._h, -1, 0, 0))      # cleared
    assert not t.seal_verify(d, good, limbs=2).any()
    eng.check()


def test_scratch_growth_between_launches_in_flight(F):
    """The context's partial-sum scratch grows while an earlier launch that uses the old block may still be in flight: one row of
    2^5 (the smallest scratch), then 8 rows of 2^12 sealed and verified, on one stream with no host synchronisation in between.
    The second seal is that of an engine whose scratch never had the small size, bit for bit."""
    from fhe_reliability_gpu_amd._lib import check, lib
    eng, fresh = F.Engine(0), F.Engine(0)
    n_poly, limbs, N = 2, 4, 1 << 12
    rows = n_poly * limbs
    qs = F.create_moduli(N, limb_bits("mixed", limbs, 0))
    qs5 = F.create_moduli(1 << 5, [50])
    t5, t12, t12_fresh = eng.tables(5, qs5), eng.tables(12, qs), fresh.tables(12, qs)
    rng = np.random.default_rng(22)
    x = np.stack([rng.integers(0, qs[r % limbs], N, dtype=np.uint64) for r in range(rows)])
    x[5, 77] = 12345                                         # small, so that the flipped bit 9 below stays below q
    d5, d, d_fresh = eng.upload(rng.integers(0, qs5[0], 1 << 5, dtype=np.uint64)), eng.upload(x), fresh.upload(x)
    s5, s, fl = eng.alloc(2), eng.alloc(2 * rows), eng.upload(np.full((rows + 1) // 2, GARBAGE, dtype=np.uint64))
    eng.sync()
    check(lib.fhe_seal(eng._h, s5.ptr, d5.ptr, t5._h, 1, 1, 0, None))
    check(lib.fhe_seal(eng._h, s.ptr, d.ptr, t12._h, n_poly, limbs, 0, None))
    check(lib.fhe_seal_verify(eng._h, d.ptr, s.ptr, t12._h, n_poly, limbs, 0, fl.ptr, None))
    got = s.download().reshape(rows, 2)
    assert got.tobytes() == t12_fresh.seal(d_fresh, limbs=limbs, n_poly=n_poly).download().tobytes()
    assert got.tolist() == py_seals(x)
    assert not fl.download().view(np.uint32)[:rows].any()
    flip(eng, d, 5 * N + 77, 9)
    assert t12.seal_verify(d, s, limbs=limbs, n_poly=n_poly).tolist() == [0] * 5 + [SUM] + [0] * 2
    eng.check()


# ---------------------------------------------------------------------------------------------------------------- composites
class Case(SealedCase):
    """a plan, its detector, seeded operands on the host and on the device, and their seals"""

    def __init__(self, F, eng, name):
        super().__init__(F, eng, PLANS[name], seed=PLANS[name][0], margin=0)
        # the seals the composites are handed are right: Python integers
        for v, s in zip(self.ops, self.seals):
            assert s.download().tolist() == py_seals(v)
        assert self.key_seal.download().tolist() == py_seals(self.key)


@pytest.fixture(scope="module")
def cases(F, eng):
    return case_cache(lambda name: Case(F, eng, name))


def _seal_blocks(flags):
    return {k: v for k, v in flags.items() if k != "checked"}


PARAMS = [("A", 0), ("A", 65537), ("B", 0), ("B", 65537)]


@pytest.mark.parametrize("name,tp", PARAMS)
def test_clean_sealed_calls_give_the_unchecked_words_no_flag_and_the_outputs_seals(F, eng, cases, name, tp):
    c = cases(name)
    ks, ab, L = c.ks, c.ab, c.L
    gal = 5
    with plain_modulus(ks, tp):
        for resc in (True, False):
            lay = ks.hmult_sealed_layout(resc)
            inner = (ks.bgv_hmult_checked_layout if tp else ks.hmult_checked_layout)(resc)
            assert [lay[k][0] for k in ("a0", "a1", "b0", "b1", "key")] == [0, L, 2 * L, 3 * L, 4 * L]
            assert lay["checked"] == 4 * L + 2 * c.dnum * c.M and lay["total"] == lay["checked"] + inner["total"]
            o0, o1, so, fl = ks.hmult_sealed(*c.d, c.dk, ab, seals=c.seals, key_seal=c.key_seal, rescale=resc)
            assert raised(fl) == [], (resc, raised(fl))
            assert sorted(fl) == ["a0", "a1", "b0", "b1", "checked", "key"] and fl["key"].shape == (c.dnum, 2, c.M)
            w0, w1 = ks.hmult(*c.d, c.dk, rescale=resc)
            assert same(o0, w0) and same(o1, w1), resc
            assert so[0].download().tolist() == py_seals(w0.download()) and so[1].download().tolist() == py_seals(w1.download())
        rl = ks.rotate_sealed_layout()
        inner = ks.bgv_checked_layout() if tp else ks.checked_layout()
        assert [rl[k][0] for k in ("c0", "c1", "key")] == [0, L, 2 * L] and rl["total"] == rl["checked"] + inner["total"]
        o0, o1, so, fl = ks.rotate_sealed(c.d[0], c.d[1], gal, c.dk, ab, seals=c.seals[:2], key_seal=c.key_seal)
        assert raised(fl) == []
        w0, w1 = ks.rotate(c.d[0], c.d[1], gal, c.dk)
        assert same(o0, w0) and same(o1, w1)
        assert so[0].download().tolist() == py_seals(w0.download()) and so[1].download().tolist() == py_seals(w1.download())
        # inputs untouched
        for dv, v in zip(c.d + [c.dk], c.ops + [c.key]):
            assert (dv.download().reshape(-1) == v.reshape(-1)).all()
    eng.check()


@pytest.mark.parametrize("name,tp", PARAMS)
def test_a_flipped_word_at_rest_passes_the_checked_call_and_raises_its_seal_row(F, eng, cases, name, tp):
    c = cases(name)
    ks, ab, L, N, M = c.ks, c.ab, c.L, c.N, c.M
    with plain_modulus(ks, tp):
        checked = ks.bgv_hmult_checked if tp else ks.hmult_checked
        rchecked = ks.bgv_rotate_checked if tp else ks.rotate_checked
        clean = [o.download() for o in ks.hmult(*c.d, c.dk)]
        rclean = [o.download() for o in ks.rotate(c.d[0], c.d[1], 5, c.dk)]
        # (operand name, its device array, row, host words of that row, modulus)
        key_row = (1 * 2 + 1) * M + (M - 1)                      # digit 1, half 1, the last special limb
        targets = [("a0", c.d[0], L - 1, c.ops[0][L - 1], c.qs[L - 1]), ("b1", c.d[3], 0, c.ops[3][0], c.qs[0]),
                   ("key", c.dk, key_row, c.key[1, 1, M - 1], c.qs[M - 1])]
        for what, dev, row, words, q in targets:
            j = safe_coeff(words, q, N // 2 + 7)
            flip(eng, dev, row * N + j, 3)
            try:
                # the gap: the checked call computes on the flipped operand and raises nothing
                o0, o1, fl = checked(*c.d, c.dk, ab)
                assert raised(fl) == [], what
                assert (o0.download() != clean[0]).any() or (o1.download() != clean[1]).any(), what
                # its closure: exactly that row of the seal blocks
                p0, p1, so, sfl = ks.hmult_sealed(*c.d, c.dk, ab, seals=c.seals, key_seal=c.key_seal)
                assert raised(_seal_blocks(sfl)) == [(what, row)], (what, raised(_seal_blocks(sfl)))
                assert int(np.asarray(sfl[what]).reshape(-1)[row]) == SUM
                assert same(p0, o0) and same(p1, o1)           # the call went on, on what it was given
                # a NULL seal skips its rows
                seals = [None if n == what else s for n, s in zip(("a0", "a1", "b0", "b1"), c.seals)]
                sfl = ks.hmult_sealed(*c.d, c.dk, ab, seals=seals, key_seal=None if what == "key" else c.key_seal)[3]
                assert raised(_seal_blocks(sfl)) == [], what
                if what in ("a0", "key"):      # a0 is the rotation's c0
                    o0, o1, fl = rchecked(c.d[0], c.d[1], 5, c.dk, ab)
                    assert raised(fl) == [] and ((o0.download() != rclean[0]).any() or (o1.download() != rclean[1]).any()), what
                    sfl = ks.rotate_sealed(c.d[0], c.d[1], 5, c.dk, ab, seals=c.seals[:2], key_seal=c.key_seal)[3]
                    assert raised(_seal_blocks(sfl)) == [("c0" if what == "a0" else "key", row)], what
            finally:
                flip(eng, dev, row * N + j, 3)
        assert raised(ks.hmult_sealed(*c.d, c.dk, ab, seals=c.seals, key_seal=c.key_seal)[3]) == []
        assert ks.hmult_sealed(*c.d, c.dk, ab)[3]["a0"].tolist() == [0] * L      # no seal at all: nothing verified
    eng.check()


@pytest.mark.parametrize("name,tp", PARAMS)
def test_the_checked_calls_hook_fires_in_the_embedded_block_and_the_chain_carries_seals(F, eng, cases, name, tp):
    from fhe_reliability_gpu_amd._lib import check, lib
    c = cases(name)
    ks, ab, L, N = c.ks, c.ab, c.L, c.N
    arm = lib.fhe_ctx_inject_fault_bgv_keyswitch if tp else lib.fhe_ctx_inject_fault_keyswitch
    with plain_modulus(ks, tp):
        # stage 7 (tail), the word before its window check, unit 1: its own word of the embedded block, nothing in the seal blocks
        check(arm(eng._h, 7, 2, 1, 3, 30))
        fl = ks.hmult_sealed(*c.d, c.dk, ab, seals=c.seals, key_seal=c.key_seal)[3]
        assert raised(fl) == [("checked.keyswitch.tail", 1)], raised(fl)
        check(arm(eng._h, 7, 2, L + 1, 3, 30))
        fl = ks.rotate_sealed(c.d[0], c.d[1], 5, c.dk, ab, seals=c.seals[:2], key_seal=c.key_seal)[3]
        assert raised(fl) == [("checked.tail", L + 1)], raised(fl)
        # the chain: a multiply's sealed output, one bit flipped at rest, into a sealed rotation
        o0, o1, so, fl = ks.hmult_sealed(*c.d, c.dk, ab, seals=c.seals, key_seal=c.key_seal, rescale=False)
        assert raised(fl) == []
        assert raised(ks.rotate_sealed(o0, o1, 5, c.dk, ab, seals=so, key_seal=c.key_seal)[3]) == []
        host = o1.download()
        row = L - 1
        j = safe_coeff(host[row], c.qs[row], 11)
        flip(eng, o1, row * N + j, 3)
        fl = ks.rotate_sealed(o0, o1, 5, c.dk, ab, seals=so, key_seal=c.key_seal)[3]
        assert raised(_seal_blocks(fl)) == [("c1", row)]
    eng.check()


def test_scope_errors_are_the_checked_calls_statuses_with_nothing_launched(F, eng, cases):
    from fhe_reliability_gpu_amd._lib import check, lib, vp
    c = cases("A")
    ks, ab, N, L, K = c.ks, c.ab, c.N, c.L, c.K
    o0, o1 = eng.alloc(L * N), eng.alloc(L * N)
    words = (ks.hmult_sealed_layout(True)["total"] + 1) // 2 + 64
    sin = (vp * 4)(*[s.ptr for s in c.seals])
    d = c.d

    def both(plan, abft, flags):
        return [lib.fhe_hmult_sealed(eng._h, plan, o0.ptr, o1.ptr, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, c.dk.ptr, 1, abft, sin, c.key_seal.ptr, None,
                                     flags, None),
                lib.fhe_rotate_sealed(eng._h, plan, o0.ptr, o1.ptr, d[0].ptr, d[1].ptr, 5, c.dk.ptr, abft, sin, c.key_seal.ptr, None, flags, None)]

    def refused(plan, abft, status, why):
        fl = eng.upload(np.full(words, GARBAGE, dtype=np.uint64))
        assert both(plan, abft, fl.ptr) == [status] * 2 and why in lib.fhe_last_error().decode()
        assert (fl.download() == GARBAGE).all()      # nothing launched, not even a verification

    fl = eng.upload(np.full(words, GARBAGE, dtype=np.uint64))
    assert both(ks._h, ab._h, fl.ptr) == [0, 0]
    # a one-rank sharded plan
    g1, g2, bc = eng.alloc(L * N), eng.alloc(2 * K * N), eng.alloc(3 * N)
    sh = vp()
    check(lib.fhe_keyswitch_create_sharded(eng._h, c.t._h, L, K, c.dnum, 1, 0, g1.ptr, g2.ptr, bc.ptr, C.byref(sh)))
    try:
        refused(sh, ab._h, INVALID, "sharded")
        check(lib.fhe_keyswitch_set_plain_modulus(sh, 65537))
        refused(sh, ab._h, INVALID, "sharded")
    finally:
        lib.fhe_keyswitch_destroy(sh)
    # a detector made for another table set; no detector; no flags
    ab2 = F.Abft(eng, eng.tables(c.logn, c.qs))
    refused(ks._h, ab2._h, INVALID, "another table set")
    refused(ks._h, None, INVALID, "null")
    assert both(ks._h, ab._h, None) == [INVALID] * 2
    # ntt_mode = 1, on both forms
    for tp in (0, 65537):
        with plain_modulus(ks, tp):
            eng.set_option("ntt_mode", 1)
            try:
                refused(ks._h, ab._h, UNSUPPORTED, "ntt_mode")
            finally:
                eng.set_option("ntt_mode", 0)
            assert both(ks._h, ab._h, fl.ptr) == [0, 0]
    # an even Galois element, equal output parts
    assert lib.fhe_rotate_sealed(eng._h, ks._h, o0.ptr, o1.ptr, d[0].ptr, d[1].ptr, 4, c.dk.ptr, ab._h, sin, None, None, fl.ptr, None) == INVALID
    assert lib.fhe_hmult_sealed(eng._h, ks._h, o0.ptr, o0.ptr, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, c.dk.ptr, 1, ab._h, sin, None, None, fl.ptr, None) == INVALID
    eng.check()
