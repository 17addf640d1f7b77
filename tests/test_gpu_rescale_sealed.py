"""The rescale / mod switch whose input is verified on the loads that consume it and whose output is sealed from the registers that
are stored (rescale_sealed), on the GPU: the words are rescale's, the output seals are NttTables.seal's, a corruption at rest
raises exactly its input row, and -- what only this call can see -- a fault on the tail's own load of an input word raises that
row's seal word while the residue identity, formed from the word as loaded, stays silent; a fault after the output's digest is
caught by the next verification.

Plans (logn, L, K, dnum) as test_gpu_ntt_sealed.py: A (10, 4, 2, 2), a row shorter than a chunk; B (13, 3, 1, 3) with a 61-bit prime
among 50-bit ones, one chunk per row; C (14, 6, 2, 3), two chunks per row.  Each without and with plain modulus 65537.  Operands
are drawn from [16, q - 16), so that bit-3 flips stay below q."""
import ctypes as C

import numpy as np
import pytest

from helpers.sealed_case import case_cache, flip, plain_modulus, plans, raised, sealed_plan

pytestmark = pytest.mark.gpu

INVALID = 1
SUM, RANGE = 1, 2
PW_OPERAND = 4
LOAD, STORE = 0, 1
GARBAGE = 0x5A5A5A5A5A5A5A5A
PLANS = plans("ABC")
PARAMS = [(name, tp) for name in PLANS for tp in (0, 65537)]
CHUNK = 8192


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


class Case:
    """a plan, its detector, a seeded three-part input on the host and on the device, and its seal"""

    def __init__(self, F, eng, name):
        self.logn, self.L, self.K, self.dnum, _ = PLANS[name]
        self.N, self.R = 1 << self.logn, self.L - 1
        self.qs, self.t, self.ks, self.ab = sealed_plan(F, eng, PLANS[name])
        rng = np.random.default_rng(311 + self.logn + self.dnum)
        self.c = np.stack([np.stack([rng.integers(16, q - 16, self.N, dtype=np.uint64) for q in self.qs[:self.L]]) for _ in range(3)])
        self.d = eng.upload(self.c)
        self.seal = self.t.seal(self.d, limbs=self.L, n_poly=3)
        self.edge = CHUNK if self.N > CHUNK else self.N // 2
        self.ref = {}       # (form, n_parts) -> (words, seal) of the unchecked rescale, computed once

    def reference(self, tp, n):
        if (tp, n) not in self.ref:
            o = self.ks.rescale(self.d, n)
            self.ref[(tp, n)] = (o.download().reshape(n, self.R, self.N), self.t.seal(o, limbs=self.R, n_poly=n).download().reshape(n, self.R, 2))
        return self.ref[(tp, n)]

    def words(self):
        return [0, self.edge - 1, self.edge, self.N - 1]

    def unchanged(self):
        return (self.d.download().reshape(-1) == self.c.reshape(-1)).all()


@pytest.fixture(scope="module")
def cases(F, eng):
    return case_cache(lambda name: Case(F, eng, name))


def words_of(o, c, n):
    return o.download().reshape(n, c.R, c.N)


def seal_of(s, c, n):
    return s.download().reshape(n, c.R, 2)


@pytest.mark.parametrize("name,tp", PARAMS)
def test_clean_words_seals_and_flags(F, eng, cases, name, tp):
    c = cases(name)
    with plain_modulus(c.ks, tp):
        for n in (1, 2, 3):
            lay = c.ks.rescale_sealed_layout(n)
            inner = c.ks.bgv_mod_switch_checked_layout(n) if tp else c.ks.rescale_checked_layout(n)
            assert lay["in"] == (0, (n, c.L)) and lay["checked"] == n * c.L and lay["total"] == n * c.L + inner["total"]
            want, want_seal = c.reference(tp, n)
            o, so, fl = c.ks.rescale_sealed(c.d, c.ab, c.seal, n)
            assert raised(fl) == [], (n, raised(fl))
            assert (words_of(o, c, n) == want).all(), n
            assert (seal_of(so, c, n) == want_seal).all(), n
            assert fl["in"].shape == (n, c.L) and set(fl["checked"]) == set(inner) - {"total"}
        assert c.unchanged()
    eng.check()


@pytest.mark.parametrize("name,tp", PARAMS)
def test_a_corruption_at_rest_raises_exactly_its_input_row(F, eng, cases, name, tp):
    c = cases(name)
    n = 2
    with plain_modulus(c.ks, tp):
        for row in (0, c.L + c.L - 2, c.L - 1):      # row 0, row L - 2 of the last part, a last-limb row
            for j in c.words():
                flip(eng, c.d, row * c.N + j, 3)
                try:
                    o, so, fl = c.ks.rescale_sealed(c.d, c.ab, c.seal, n)
                    want = c.ks.rescale(c.d, n)
                finally:
                    flip(eng, c.d, row * c.N + j, 3)
                assert raised(fl) == [("in", row)] and int(fl["in"].reshape(-1)[row]) == SUM, (row, j, raised(fl))
                assert (o.download() == want.download()).all(), (row, j)      # the rescale of the input as it is
                assert (seal_of(so, c, n) == seal_of(c.t.seal(want, limbs=c.R, n_poly=n), c, n)).all(), (row, j)
        assert c.unchanged()
    eng.check()


@pytest.mark.parametrize("name,tp", PARAMS)
def test_a_word_not_below_q_raises_the_window_and_the_operand_bit(F, eng, cases, name, tp):
    c = cases(name)
    n = 2
    with plain_modulus(c.ks, tp):
        for row, j in ((c.L + 1, c.edge), (c.L - 1, c.edge - 1)):
            bad = c.c.copy()
            bad.reshape(-1)[row * c.N + j] = GARBAGE
            db = eng.upload(bad)
            o, so, fl = c.ks.rescale_sealed(db, c.ab, c.seal, n)
            assert int(fl["in"].reshape(-1)[row]) & RANGE and [u for nm, u in raised(fl) if nm == "in"] == [row], (row, raised(fl))
            part, l = divmod(row, c.L)
            if l < c.R:      # the checked tail sees the word: PW_OPERAND on its unit and nothing else
                assert raised(fl["checked"]) == [("scale", part * c.R + l)] and int(fl["checked"]["scale"][part, l]) == PW_OPERAND
                assert (o.download() == c.ks.rescale(db, n).download()).all()      # flagged, not fixed
    eng.check()


@pytest.mark.parametrize("name,tp", PARAMS)
def test_a_fault_on_the_tails_own_load_is_seen_by_the_sealed_call_only(F, eng, cases, name, tp):
    c = cases(name)
    n = 2
    with plain_modulus(c.ks, tp):
        want, want_seal = c.reference(tp, n)
        for row, j in ((1, c.edge - 1), (c.L + c.L - 2, c.edge)):
            part, l = divmod(row, c.L)
            eng.inject_fault_subscale_sealed(LOAD, row, j, 3)
            # the checked rescale does not run the sealed tail: it sees nothing and leaves the hook armed
            oc, fc = c.ks.bgv_mod_switch_checked(c.d, c.ab, n) if tp else c.ks.rescale_checked(c.d, c.ab, n)
            assert raised(fc) == [] and (words_of(oc, c, n) == want).all()
            o, so, fl = c.ks.rescale_sealed(c.d, c.ab, c.seal, n)
            assert raised(fl) == [("in", row)] and int(fl["in"][part, l]) == SUM, (row, j, raised(fl))      # stage 3's residue words stay zero
            assert c.unchanged()                                                                              # memory is clean
            diff = np.argwhere(words_of(o, c, n) != want)
            assert diff.tolist() == [[part, l, j]], (row, j, diff.tolist())                                   # the gap, shown
            o, so, fl = c.ks.rescale_sealed(c.d, c.ab, c.seal, n)                                             # one shot
            assert raised(fl) == [] and (words_of(o, c, n) == want).all() and (seal_of(so, c, n) == want_seal).all()
    eng.check()


@pytest.mark.parametrize("name,tp", PARAMS)
def test_a_fault_after_the_digest_is_caught_by_the_next_verification(F, eng, cases, name, tp):
    c = cases(name)
    with plain_modulus(c.ks, tp):
        for n, row, j in ((2, c.R + 1, c.edge), (3, 2 * c.R + c.R - 1, c.N - 1), (1, 0, 0)):
            want, want_seal = c.reference(tp, n)
            part, l = divmod(row, c.R)
            eng.inject_fault_subscale_sealed(STORE, row, j, 3)
            o, so, fl = c.ks.rescale_sealed(c.d, c.ab, c.seal, n)
            assert raised(fl) == []
            assert (seal_of(so, c, n) == want_seal).all()                   # the seal of the fault-free output
            got = words_of(o, c, n)
            assert np.argwhere(got != want).tolist() == [[part, l, j]] and int(got[part, l, j]) == int(want[part, l, j]) ^ 8
            v = c.t.seal_verify(o, so, limbs=c.R, n_poly=n)
            assert np.flatnonzero(np.asarray(v).reshape(-1)).tolist() == [row]
            assert raised(c.ks.rescale_sealed(c.d, c.ab, c.seal, n)[2]) == []      # one shot
        assert c.unchanged()
    eng.check()


@pytest.mark.parametrize("name,tp", PARAMS)
def test_the_transforms_hook_on_a_last_limb_row_raises_that_row_and_no_abft_word(F, eng, cases, name, tp):
    c = cases(name)
    n = 2
    with plain_modulus(c.ks, tp):
        want, _ = c.reference(tp, n)
        row = c.L + c.L - 1
        eng.inject_fault_ntt_sealed(row, c.edge + 1, 3)
        o, so, fl = c.ks.rescale_sealed(c.d, c.ab, c.seal, n)
        assert raised(fl) == [("in", row)] and int(fl["in"].reshape(-1)[row]) == SUM, raised(fl)
        got = words_of(o, c, n)
        assert not (got[1] == want[1]).all() and (got[0] == want[0]).all()
        assert c.unchanged()
        # not a last-limb row: refused, and gone afterwards
        from fhe_reliability_gpu_amd._lib import FheError
        eng.inject_fault_ntt_sealed(1, 0, 3)
        with pytest.raises(FheError, match="last-limb"):
            c.ks.rescale_sealed(c.d, c.ab, c.seal, n)
        assert raised(c.ks.rescale_sealed(c.d, c.ab, c.seal, n)[2]) == []
    eng.check()


@pytest.mark.parametrize("name,tp", PARAMS)
def test_refusals_launch_nothing_and_take_the_hook(F, eng, cases, name, tp):
    from fhe_reliability_gpu_amd._lib import lib
    c = cases(name)
    n = 2
    with plain_modulus(c.ks, tp):
        total = c.ks.rescale_sealed_layout(n)["total"]
        o = eng.alloc(n * c.R * c.N)
        so = eng.alloc(n * c.R * 2)
        raw = lambda fl, out, seal_in: lib.fhe_rescale_sealed(eng._h, c.ks._h, out, c.d.ptr, n, c.ab._h, seal_in, so.ptr, fl.ptr, None)
        inside = C.c_void_p(c.d.ptr.value + 8 * c.N)     # an output that overlaps the input
        for arm, out, seal_in, why in ((lambda: eng.inject_fault_subscale_sealed(LOAD, n * c.L, 0, 3), o.ptr, c.seal.ptr, "outside the call"),
                                       (lambda: eng.inject_fault_subscale_sealed(STORE, n * c.R, 0, 3), o.ptr, c.seal.ptr, "outside the call"),
                                       (lambda: eng.inject_fault_subscale_sealed(STORE, 0, c.N, 3), o.ptr, c.seal.ptr, "outside the call"),
                                       (lambda: eng.inject_fault_subscale_sealed(LOAD, c.L - 1, 0, 3), o.ptr, c.seal.ptr, "last-limb"),
                                       (lambda: eng.inject_fault_subscale_sealed(LOAD, 0, 0, 3), o.ptr, None, "null"),
                                       (lambda: eng.inject_fault_subscale_sealed(LOAD, 0, 0, 3), inside, c.seal.ptr, "out of place")):
            arm()
            fl = eng.upload(np.full((total + 1) // 2 + 8, GARBAGE, dtype=np.uint64))
            assert raw(fl, out, seal_in) == INVALID and why in lib.fhe_last_error().decode(), why
            assert (fl.download() == GARBAGE).all(), why
            # the refused call took the hook: the next one is clean
            assert raw(fl, o.ptr, c.seal.ptr) == 0 and not fl.download().view(np.uint32)[:total].any(), why
        assert c.unchanged()
    eng.check()


@pytest.mark.parametrize("name,tp", PARAMS)
def test_the_checked_rescales_own_hook_raises_its_own_word_and_no_input_row(F, eng, cases, name, tp):
    from fhe_reliability_gpu_amd._lib import check, lib
    c = cases(name)
    n = 2
    arm = lib.fhe_ctx_inject_fault_bgv_mod_switch if tp else lib.fhe_ctx_inject_fault_rescale
    with plain_modulus(c.ks, tp):
        unit = c.R + 1
        check(arm(eng._h, 3, 2, unit, c.edge, 3))      # stage 3, the word before its window check
        o, so, fl = c.ks.rescale_sealed(c.d, c.ab, c.seal, n)
        assert raised(fl) == [("checked.scale", unit)], raised(fl)
        check(arm(eng._h, 1, 2, 1, 5, 3))              # stage 1, the residues
        assert raised(c.ks.rescale_sealed(c.d, c.ab, c.seal, n)[2]) == [("checked.reduce", 1)]
        assert raised(c.ks.rescale_sealed(c.d, c.ab, c.seal, n)[2]) == []
        assert c.unchanged()
    eng.check()
