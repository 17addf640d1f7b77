"""The inverse transform that verifies its input's seal on its own load (intt_sealed), and the key switch and rotation built on it
(apply_sealed_in, rotate_sealed_in), on the GPU: the words are the unchecked calls', corruptions at rest give the flags of the
compositions they replace, and -- what only these calls can see -- a fault on the transform's own load of an input word raises that
row's seal word while the ABFT identity, formed from the word as loaded, stays silent.

Plans (logn, L, K, dnum) as test_gpu_keyswitch_sealed.py: A (10, 4, 2, 2), one launch and one tile per row; B (13, 3, 1, 3) with a
61-bit prime among 50-bit ones, two tiles per row; C (14, 6, 2, 3), four tiles per row.  Each composite without and with plain
modulus 65537.  I (15, 2, 1, 2), J (16, 2, 1, 2), K (17, 2, 1, 1) with a 61-bit prime among 50-bit ones -- stage 0 above 2^14 and a
key of 4, 8 and 16 chunks per row -- through the composites' clean and at-rest tests, without plain modulus.  Operands are drawn from [16, q - 16), so that bit-3 flips stay below q."""
import ctypes as C

import numpy as np
import pytest

from helpers.sealed_case import SealedCase, case_cache, flat, flip, plain_modulus, plans, raised, same

pytestmark = pytest.mark.gpu

INVALID = 1
SUM, RANGE = 1, 2
GARBAGE = 0x5A5A5A5A5A5A5A5A
PLANS = plans("ABC")
NAMES = list(PLANS)
PARAMS = [(name, tp) for name in PLANS for tp in (0, 65537)]
BIG = [(name, 0) for name in "IJK"]
PLANS.update(plans("IJK"))
GALOIS = 5
TILE = 4096      # words per (row, tile) of the two-launch sizes' first launch


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


class Case(SealedCase):
    """a plan, its detector, seeded operands and key on the host and on the device, their seals, and the unchecked references"""

    def __init__(self, F, eng, name):
        logn, _, _, dnum, _ = PLANS[name]
        super().__init__(F, eng, PLANS[name], seed=277 + logn + dnum, margin=16, n_ops=2)
        self.rows = self.dnum * 2 * self.M
        self.edge = TILE if self.logn >= 13 else self.N // 2
        self.intt_ref = self.unchecked_intt(eng, self.d[0])      # computed once, shared

    def unchecked_intt(self, eng, src):
        w = eng.alloc(self.L * self.N)
        w.copy_from(src)
        self.t.inverse(w, limbs=self.L)
        return w.download().reshape(self.L, self.N)

    def words(self):
        """(row, word): word 0, both sides of a tile edge, the last word -- on chosen rows"""
        return [(0, 0), (1, self.edge - 1), (self.L - 1, self.edge), (self.L // 2, self.N - 1)]


@pytest.fixture(scope="module")
def cases(F, eng):
    return case_cache(lambda name: Case(F, eng, name))



# ---- the transform ----

@pytest.mark.parametrize("name", NAMES)
def test_transform_clean_words_and_flags_in_place_and_out_of_place(F, eng, cases, name):
    c = cases(name)
    dst, fl = c.t.intt_sealed(c.d[0], c.seals[0], c.ab, limbs=c.L)
    assert fl.shape == (2, c.L) and not fl.any()
    assert (dst.download().reshape(c.L, c.N) == c.intt_ref).all()
    assert c.unchanged()
    w = eng.alloc(c.L * c.N)
    w.copy_from(c.d[0])
    same_buf, fl = c.t.intt_sealed(w, c.seals[0], c.ab, dst=w, limbs=c.L)
    assert same_buf is w and not fl.any()
    assert (w.download().reshape(c.L, c.N) == c.intt_ref).all()
    # without a stored seal nothing is compared; a window of limbs and two polynomials address their own rows
    _, fl = c.t.intt_sealed(c.d[0], None, c.ab, limbs=c.L)
    assert not fl.any()
    two = eng.upload(np.stack([c.ops[0][1:], c.ops[1][1:]]))
    s2 = c.t.seal(two, limbs=c.L - 1, start=1, n_poly=2)
    dst, fl = c.t.intt_sealed(two, s2, c.ab, limbs=c.L - 1, start=1, n_poly=2)
    assert fl.shape == (2, 2 * (c.L - 1)) and not fl.any()
    assert (dst.download().reshape(2, c.L - 1, c.N)[0] == c.intt_ref[1:]).all()
    eng.check()


@pytest.mark.parametrize("name", NAMES)
def test_transform_flips_in_source_memory_raise_that_rows_seal_word_only(F, eng, cases, name):
    c = cases(name)
    src = eng.alloc(c.L * c.N)
    src.copy_from(c.d[0])
    for row, j in c.words():
        flip(eng, src, row * c.N + j, 3)
        try:
            dst, fl = c.t.intt_sealed(src, c.seals[0], c.ab, limbs=c.L)
            want = c.unchecked_intt(eng, src)
        finally:
            flip(eng, src, row * c.N + j, 3)
        assert np.flatnonzero(fl[0]).tolist() == [row] and int(fl[0][row]) == SUM and not fl[1].any(), (row, j, fl)
        assert (dst.download().reshape(c.L, c.N) == want).all(), (row, j)      # the transform of the row as it is
    # a word >= q: the window (and the sums, which see 2^63 as 4)
    row, j = c.L - 1, c.edge
    flip(eng, src, row * c.N + j, 63)
    _, fl = c.t.intt_sealed(src, c.seals[0], c.ab, limbs=c.L)
    flip(eng, src, row * c.N + j, 63)
    assert np.flatnonzero(fl[0]).tolist() == [row] and int(fl[0][row]) & RANGE and not fl[1].any()
    # without a stored seal the window is still checked
    flip(eng, src, row * c.N + j, 63)
    _, fl = c.t.intt_sealed(src, None, c.ab, limbs=c.L)
    flip(eng, src, row * c.N + j, 63)
    assert fl[0].tolist() == [RANGE if r == row else 0 for r in range(c.L)]
    # a garbage, non-canonical stored seal: that row only
    s = c.seals[0].download().copy().reshape(c.L, 2)
    s[1] = GARBAGE
    _, fl = c.t.intt_sealed(src, eng.upload(s), c.ab, limbs=c.L)
    assert fl[0].tolist() == [SUM if r == 1 else 0 for r in range(c.L)] and not fl[1].any()
    s = c.seals[0].download().copy().reshape(c.L, 2)
    s[0, 0] += np.uint64((1 << 61) - 1)      # the same residue, not canonical
    _, fl = c.t.intt_sealed(src, eng.upload(s), c.ab, limbs=c.L)
    assert fl[0].tolist() == [SUM] + [0] * (c.L - 1)
    _, fl = c.t.intt_sealed(src, c.seals[0], c.ab, limbs=c.L)
    assert not fl.any()
    eng.check()


@pytest.mark.parametrize("name", ["B", "C"])
def test_transform_flip_between_the_launches_raises_the_abft_word_and_no_seal_word(F, eng, cases, name):
    from fhe_reliability_gpu_amd._lib import check, lib
    c = cases(name)
    row, j = 1, c.edge + 5
    check(lib.fhe_ctx_inject_fault(eng._h, row * c.N + j, 30))
    dst, fl = c.t.intt_sealed(c.d[0], c.seals[0], c.ab, limbs=c.L)
    assert not fl[0].any() and np.flatnonzero(fl[1]).tolist() == [row]
    assert not (dst.download().reshape(c.L, c.N) == c.intt_ref).all()
    dst, fl = c.t.intt_sealed(c.d[0], c.seals[0], c.ab, limbs=c.L)      # one shot
    assert not fl.any() and (dst.download().reshape(c.L, c.N) == c.intt_ref).all()
    assert c.unchanged()
    eng.check()


# ---- the gap, shown ----

@pytest.mark.parametrize("name", NAMES)
def test_a_fault_on_the_transforms_own_load_is_seen_by_the_sealed_transform_only(F, eng, cases, name):
    c = cases(name)
    for row, j in c.words():
        # the composition: a verifying sweep, then the checked inverse on a copy -- it does not run the sealed transform, leaves
        # the hook armed and sees nothing
        eng.inject_fault_ntt_sealed(row, j, 3)
        w = eng.alloc(c.L * c.N)
        w.copy_from(c.d[0])
        assert not c.t.seal_verify(c.d[0], c.seals[0], limbs=c.L).any()
        assert not c.ab.inverse_checked(w, limbs=c.L).any()
        assert (w.download().reshape(c.L, c.N) == c.intt_ref).all()
        dst, fl = c.t.intt_sealed(c.d[0], c.seals[0], c.ab, limbs=c.L)
        assert np.flatnonzero(fl[0]).tolist() == [row] and int(fl[0][row]) == SUM, (row, j, fl)
        assert not fl[1].any(), (row, j)                                  # a consistent input of the ABFT identity
        assert c.unchanged()                                              # memory is clean
        got = dst.download().reshape(c.L, c.N)
        assert not (got[row] == c.intt_ref[row]).all() and (np.delete(got, row, 0) == np.delete(c.intt_ref, row, 0)).all()
        dst, fl = c.t.intt_sealed(c.d[0], c.seals[0], c.ab, limbs=c.L)    # one shot
        assert not fl.any() and (dst.download().reshape(c.L, c.N) == c.intt_ref).all()
    # a hook outside the call: refused with nothing launched, and gone afterwards
    from fhe_reliability_gpu_amd._lib import lib
    for bad in ((c.L, 0, 3), (0, c.N, 3)):
        eng.inject_fault_ntt_sealed(*bad)
        fl = eng.upload(np.full(c.L + 8, GARBAGE, dtype=np.uint64))
        dst = eng.alloc(c.L * c.N)
        rc = lib.fhe_ntt_inverse_sealed(eng._h, dst.ptr, c.d[0].ptr, c.t._h, c.ab._h, 1, c.L, 0, c.seals[0].ptr, fl.ptr, None)
        assert rc == INVALID and "outside the call" in lib.fhe_last_error().decode()
        assert (fl.download() == GARBAGE).all()
        assert not c.t.intt_sealed(c.d[0], c.seals[0], c.ab, limbs=c.L)[1].any()
    eng.inject_fault_ntt_sealed(0, 0, 3)
    eng.inject_fault_ntt_sealed(-1)                                       # disarmed
    assert not c.t.intt_sealed(c.d[0], c.seals[0], c.ab, limbs=c.L)[1].any()
    eng.check()


def test_intt_sealed_is_intt_sealed_out_without_an_output_seal(F, eng):
    """One host body and one launcher serve both calls: at the largest single-pass size and the smallest two-launch size, with a
    50-bit and a 61-bit prime (both arithmetic paths), words and flags are equal on clean rows and on a hooked row of either path."""
    for logn in (12, 13):
        N = 1 << logn
        qs = F.create_moduli(N, [50, 61])
        t = eng.tables(logn, qs)
        ab = F.Abft(eng, t)
        rng = np.random.default_rng(500 + logn)
        d = eng.upload(np.stack([rng.integers(16, q - 16, N, dtype=np.uint64) for q in qs]))
        seal = t.seal(d)
        for hit in (None, (0, N // 2 + 1, 3), (1, N - 1, 3)):
            if hit:
                eng.inject_fault_ntt_sealed(*hit)
            a, fa = t.intt_sealed(d, seal, ab)
            if hit:
                eng.inject_fault_ntt_sealed(*hit)
            b, no_seal, fb = t.intt_sealed_out(d, seal, ab, seal_out=False)
            assert no_seal is None and fa.shape == fb.shape == (2, 2)
            assert (fa == fb).all() and not fa[1].any(), (logn, hit, fa, fb)
            assert fa[0].tolist() == [SUM if hit and r == hit[0] else 0 for r in range(2)], (logn, hit, fa)
            assert (a.download() == b.download()).all(), (logn, hit)
    eng.check()


# ---- apply_sealed_in ----

def swept_apply(c, tp):
    """the composition apply_sealed_in replaces: a sweep over c's rows, then apply_sealed -- in apply_sealed_in's structure"""
    cf = c.t.seal_verify(c.d[0], c.seals[0], limbs=c.L)
    o0, o1, fl = c.ks.apply_sealed(c.d[0], c.dk, c.ab, key_seal=c.key_seal)
    return o0, o1, {"c": np.asarray(cf), "key": fl["key"], "checked": fl["checked"]}


@pytest.mark.parametrize("name,tp", PARAMS + BIG)
def test_apply_sealed_in_clean_and_corrupted_at_rest(F, eng, cases, name, tp):
    c = cases(name)
    ks, ab = c.ks, c.ab
    with plain_modulus(ks, tp):
        lay = ks.apply_sealed_in_layout()
        inner = ks.apply_sealed_layout()
        assert lay["c"] == (0, (c.L,)) and lay["key"] == (c.L, (c.dnum, 2, c.M)) and lay["checked"] == c.L + c.rows
        assert lay["total"] == c.L + inner["total"] and lay["fused"] == inner["fused"]
        o0, o1, fl = ks.apply_sealed_in(c.d[0], c.dk, ab, c.seals[0], key_seal=c.key_seal)
        assert raised(fl) == []
        w0, w1 = ks.apply(c.d[0], c.dk)
        assert same(o0, w0) and same(o1, w1)
        s0, s1, sf = swept_apply(c, tp)
        assert flat(fl) == flat(sf)
        a0, a1, fl = ks.apply_sealed_in(c.d[0], c.dk, ab, c.seals[0], key_seal=c.key_seal, add0=c.d[1], add1=c.d[0])
        r0, r1, _ = ks.apply_sealed(c.d[0], c.dk, ab, key_seal=c.key_seal, add0=c.d[1], add1=c.d[0])
        assert raised(fl) == [] and same(a0, r0) and same(a1, r1)
        # c corrupted at rest: the flags of the sweep followed by apply_sealed, and apply_sealed's words on the same memory
        for row, j in c.words()[1:3]:
            flip(eng, c.d[0], row * c.N + j, 3)
            try:
                o0, o1, fl = ks.apply_sealed_in(c.d[0], c.dk, ab, c.seals[0], key_seal=c.key_seal)
                s0, s1, sf = swept_apply(c, tp)
            finally:
                flip(eng, c.d[0], row * c.N + j, 3)
            assert flat(fl) == flat(sf) and raised(fl) == [("c", row)] and int(fl["c"][row]) == SUM, (row, j, raised(fl))
            assert same(o0, s0) and same(o1, s1)
        assert c.unchanged()
    eng.check()


@pytest.mark.parametrize("name,tp", PARAMS)
def test_apply_sealed_in_hooks_and_refusals(F, eng, cases, name, tp):
    from fhe_reliability_gpu_amd._lib import lib
    c = cases(name)
    ks, ab = c.ks, c.ab
    with plain_modulus(ks, tp):
        clean = ks.apply_sealed_in(c.d[0], c.dk, ab, c.seals[0], key_seal=c.key_seal)
        row, j = c.words()[2]
        eng.inject_fault_ntt_sealed(row, j, 3)
        got = swept_apply(c, tp)                     # does not run the sealed transform: sees nothing, leaves the hook armed
        assert raised(got[2]) == [] and same(got[0], clean[0])
        o0, o1, fl = ks.apply_sealed_in(c.d[0], c.dk, ab, c.seals[0], key_seal=c.key_seal)
        assert raised(fl) == [("c", row)] and int(fl["c"][row]) == SUM, raised(fl)      # stage 0's ABFT words stay zero
        assert c.unchanged()
        assert not (same(o0, clean[0]) and same(o1, clean[1]))
        again = ks.apply_sealed_in(c.d[0], c.dk, ab, c.seals[0], key_seal=c.key_seal)
        assert raised(again[2]) == [] and same(again[0], clean[0]) and same(again[1], clean[1])
        # the key's hook still raises exactly its key row
        krow = (1 * 2 + 1) * c.M + 1
        eng.inject_fault_keyswitch_sealed(krow, 7, 3)
        assert raised(ks.apply_sealed_in(c.d[0], c.dk, ab, c.seals[0], key_seal=c.key_seal)[2]) == [("key", krow)]
        # a hook outside the call, and a null input seal: refused with nothing launched, the flag buffer untouched, the hook taken
        total = ks.apply_sealed_in_layout()["total"]
        o = (eng.alloc(c.L * c.N), eng.alloc(c.L * c.N))
        raw = lambda fl, seal_c: lib.fhe_keyswitch_apply_sealed_in(eng._h, ks._h, o[0].ptr, o[1].ptr, c.d[0].ptr, c.dk.ptr, None, None, ab._h, seal_c,
                                                                  c.key_seal.ptr, fl.ptr, None)
        for arm, seal_c, why in ((lambda: eng.inject_fault_ntt_sealed(c.L, 0, 3), c.seals[0].ptr, "outside the call"),
                                 (lambda: eng.inject_fault_ntt_sealed(0, c.N, 3), c.seals[0].ptr, "outside the call"),
                                 (lambda: eng.inject_fault_ntt_sealed(0, 0, 3), None, "null")):
            arm()
            fl = eng.upload(np.full((total + 1) // 2 + 8, GARBAGE, dtype=np.uint64))
            assert raw(fl, seal_c) == INVALID and why in lib.fhe_last_error().decode()
            assert (fl.download() == GARBAGE).all()
            assert raw(fl, c.seals[0].ptr) == 0 and not fl.download().view(np.uint32)[:total].any()
    eng.check()


# ---- rotate_sealed_in ----

@pytest.mark.parametrize("name,tp", PARAMS + BIG)
def test_rotate_sealed_in(F, eng, cases, name, tp):
    c = cases(name)
    ks, ab, L, N = c.ks, c.ab, c.L, c.N
    with plain_modulus(ks, tp):
        kw = dict(seals=c.seals[:2], key_seal=c.key_seal)
        lay = ks.rotate_sealed_in_layout()
        assert [lay[n][0] for n in ("c0", "c1", "sigma_c1", "key")] == [0, L, 2 * L, 3 * L] and lay["checked"] == 3 * L + c.rows
        clean = ks.rotate_sealed_in(c.d[0], c.d[1], GALOIS, c.dk, ab, **kw)
        assert raised(clean[3]) == []
        w0, w1 = ks.rotate(c.d[0], c.d[1], GALOIS, c.dk)
        assert same(clean[0], w0) and same(clean[1], w1)
        ref = ks.rotate_sealed_fused(c.d[0], c.d[1], GALOIS, c.dk, ab, **kw)
        assert all(same(s, r) for s, r in zip(clean[2], ref[2]))
        assert flat(clean[3]["checked"]) == flat(ref[3]["checked"]) and flat({"key": clean[3]["key"]}) == flat({"key": ref[3]["key"]})
        inputs = lambda fl: [(n, u) for n, u in raised(fl) if not n.startswith("checked")]
        row, j = c.words()[2]
        # c1 corrupted at rest: its row, and through the carried S0 sigma(c1)'s row
        flip(eng, c.d[1], row * N + j, 3)
        try:
            fl = ks.rotate_sealed_in(c.d[0], c.d[1], GALOIS, c.dk, ab, **kw)[3]
        finally:
            flip(eng, c.d[1], row * N + j, 3)
        assert inputs(fl) == [("c1", row), ("sigma_c1", row)], raised(fl)
        # c0 corrupted: its row only
        flip(eng, c.d[0], row * N + j, 3)
        try:
            fl = ks.rotate_sealed_in(c.d[0], c.d[1], GALOIS, c.dk, ab, **kw)[3]
        finally:
            flip(eng, c.d[0], row * N + j, 3)
        assert raised(fl) == [("c0", row)], raised(fl)
        # the transform's hook on sigma(c1)'s load: sigma(c1)'s row only
        eng.inject_fault_ntt_sealed(row, j, 3)
        got = ks.rotate_sealed_in(c.d[0], c.d[1], GALOIS, c.dk, ab, **kw)
        assert raised(got[3]) == [("sigma_c1", row)] and int(got[3]["sigma_c1"][row]) == SUM, raised(got[3])
        assert not (same(got[0], clean[0]) and same(got[1], clean[1]))
        # the key's hook still raises exactly its key row
        krow = (0 * 2 + 1) * c.M + 2
        eng.inject_fault_keyswitch_sealed(krow, 9, 3)
        assert raised(ks.rotate_sealed_in(c.d[0], c.d[1], GALOIS, c.dk, ab, **kw)[3]) == [("key", krow)]
        again = ks.rotate_sealed_in(c.d[0], c.d[1], GALOIS, c.dk, ab, **kw)
        assert raised(again[3]) == [] and same(again[0], clean[0]) and same(again[1], clean[1])
        assert c.unchanged()
    eng.check()
