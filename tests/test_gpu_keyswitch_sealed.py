"""The key switch with its key verified on the load that multiplies it (apply_sealed, rotate_sealed_fused, hmult_sealed_fused_key) on
the GPU: the words are the unchecked calls', and for corruptions at rest the flag buffer, the output words and the output seals are
the sweep-based calls', word for word.  What only the fused calls can see: a fault on the inner product's own load of a key word.

Plans (logn, L, K, dnum): A (10, 4, 2, 2); B (13, 3, 1, 3) with a 61-bit prime among 50-bit ones; C (14, 6, 2, 3), two chunks per row;
D (10, 13, 1, 13), one digit more than the fused kernel is instantiated for: the sweep followed by the checked inner product.  Each
without and with plain modulus 65537.  E to H (5, d, 1, d) for d = 5, 8, 9, 12, a 61-bit prime among 50-bit ones: both edges of the
instantiations for up to 8 and up to 12 digits, in the clean, the at-rest and the multiplying-load tests, without plain modulus.
I (15, 2, 1, 2), J (16, 2, 1, 2), K (17, 2, 1, 1), a 61-bit prime among 50-bit ones: 4, 8 and 16 chunks per row -- stage 0 above
2^14, the sealed inner product over more than two chunks, its finish merging 4, 8 and 16 partials -- in the same three tests.  Operands and key words are drawn from [16, q - 16), so that bit-3 flips stay below q."""
import ctypes as C

import numpy as np
import pytest

from helpers.sealed_case import CAP, CHUNK, SealedCase, case_cache, flat, flip, plain_modulus, plans, py_seals, raised, same, same_call

pytestmark = pytest.mark.gpu

INVALID = 1
SUM, RANGE = 1, 2
GARBAGE = 0x5A5A5A5A5A5A5A5A
PLANS = plans("ABCD")
PARAMS = [(name, tp) for name in PLANS for tp in (0, 65537)]
BANDS = [(name, 0) for name in "EFGHIJK"]
PLANS.update(plans("EFGHIJK"))
FUSED = [(name, tp) for name, tp in PARAMS if name != "D"]
GALOIS = 5


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


class Case(SealedCase):
    """a plan, its detector, seeded operands and key on the host and on the device, and their seals"""

    def __init__(self, F, eng, name):
        logn, _, _, dnum, _ = PLANS[name]
        super().__init__(F, eng, PLANS[name], seed=177 + logn + dnum, margin=16)
        self.alpha = -(-self.L // self.dnum)
        self.rows = self.dnum * 2 * self.M
        sample = [0, self.rows - 1, (self.rows // 2) | 1]
        got = self.key_seal.download().reshape(self.rows, 2)
        assert [got[r].tolist() for r in sample] == [py_seals(self.key.reshape(self.rows, self.N)[r:r + 1])[0] for r in sample]
        self.fused = self.dnum <= CAP

    def key_row(self, d, h, j):
        return (d * 2 + h) * self.M + j

    def key_words(self):
        """(key row, word): the key's first word, both sides of a chunk edge (of the row's middle below two chunks), the last word of
        the last special limb of the last digit's half 1, and a word of a row inside its digit's own limb range; above two chunks per
        row also both sides of the last chunk edge"""
        edge = CHUNK if self.logn > 13 else self.N // 2
        d = self.dnum - 1
        own = min(d * self.alpha, self.L - 1)
        out = [(0, 0), (self.key_row(0, 1, 1), edge - 1), (self.key_row(d // 2, 0, self.M - 1), edge), (self.rows - 1, self.N - 1), (self.key_row(d, 0, own), 9)]
        if self.N > 2 * CHUNK:
            out += [(self.key_row(d, 1, 0), self.N - CHUNK - 1), (self.key_row(0, 0, self.M - 1), self.N - CHUNK)]
        return out


@pytest.fixture(scope="module")
def cases(F, eng):
    return case_cache(lambda name: Case(F, eng, name))


def swept_apply(c, tp, key_seal=None):
    """the composition apply_sealed replaces: a sweep over the key's rows, then the checked key switch -- in apply_sealed's structure"""
    kf = c.t.seal_verify(c.dk, c.key_seal if key_seal is None else key_seal, limbs=c.M, n_poly=2 * c.dnum)
    o0, o1, cf = (c.ks.bgv_apply_checked if tp else c.ks.apply_checked)(c.d[0], c.dk, c.ab)
    return o0, o1, {"key": np.asarray(kf).reshape(c.dnum, 2, c.M), "checked": cf}


@pytest.mark.parametrize("name,tp", PARAMS + BANDS)
def test_clean_words_flags_and_seals_are_the_sweep_based_calls(F, eng, cases, name, tp):
    c = cases(name)
    ks, ab = c.ks, c.ab
    with plain_modulus(ks, tp):
        lay = ks.apply_sealed_layout()
        assert lay["key"] == (0, (c.dnum, 2, c.M)) and lay["checked"] == c.rows and lay["fused"] == c.fused
        assert lay["total"] == c.rows + (ks.bgv_checked_layout() if tp else ks.checked_layout())["total"]
        o0, o1, fl = ks.apply_sealed(c.d[0], c.dk, ab, key_seal=c.key_seal)      # the flag buffer starts out as garbage (engine._flag_buffer)
        assert raised(fl) == [] and fl["key"].shape == (c.dnum, 2, c.M)
        w0, w1 = ks.apply(c.d[0], c.dk)
        assert same(o0, w0) and same(o1, w1)
        s0, s1, sf = swept_apply(c, tp)
        assert flat(fl) == flat(sf) and same(o0, s0) and same(o1, s1)
        # with addends, and without a stored seal: the same words, nothing raised
        a0, a1, fl = ks.apply_sealed(c.d[0], c.dk, ab, add0=c.d[1], add1=c.d[2])
        r0, r1, _ = (ks.bgv_apply_checked if tp else ks.apply_checked)(c.d[0], c.dk, ab, add0=c.d[1], add1=c.d[2])
        assert raised(fl) == [] and same(a0, r0) and same(a1, r1)
        kw = dict(seals=c.seals[:2], key_seal=c.key_seal)
        assert same_call(ks.rotate_sealed_fused(c.d[0], c.d[1], GALOIS, c.dk, ab, **kw), ks.rotate_sealed(c.d[0], c.d[1], GALOIS, c.dk, ab, **kw))
        w0, w1 = ks.rotate(c.d[0], c.d[1], GALOIS, c.dk)
        got = ks.rotate_sealed_fused(c.d[0], c.d[1], GALOIS, c.dk, ab, **kw)
        assert raised(got[3]) == [] and same(got[0], w0) and same(got[1], w1)
        for resc in ((True, False) if name == "A" else (True,)):
            kw = dict(seals=c.seals, key_seal=c.key_seal, rescale=resc)
            got = ks.hmult_sealed_fused_key(*c.d, c.dk, ab, **kw)
            assert raised(got[3]) == [] and same_call(got, ks.hmult_sealed(*c.d, c.dk, ab, **kw))
            w0, w1 = ks.hmult(*c.d, c.dk, rescale=resc)
            assert same(got[0], w0) and same(got[1], w1)
        assert c.unchanged()
    eng.check()


@pytest.mark.parametrize("name,tp", PARAMS + BANDS)
def test_corruptions_at_rest_in_the_key_give_the_sweep_based_calls_flags_and_words(F, eng, cases, name, tp):
    c = cases(name)
    ks, ab, N = c.ks, c.ab, c.N
    with plain_modulus(ks, tp):
        def all_calls(key_seal):
            rk = dict(seals=c.seals[:2], key_seal=key_seal)
            hk = dict(seals=c.seals, key_seal=key_seal, rescale=True)
            return ((ks.apply_sealed(c.d[0], c.dk, ab, key_seal=key_seal), swept_apply(c, tp, key_seal)),
                    (ks.rotate_sealed_fused(c.d[0], c.d[1], GALOIS, c.dk, ab, **rk), ks.rotate_sealed(c.d[0], c.d[1], GALOIS, c.dk, ab, **rk)),
                    (ks.hmult_sealed_fused_key(*c.d, c.dk, ab, **hk), ks.hmult_sealed(*c.d, c.dk, ab, **hk)))

        def check_all(pairs, row, where):
            (fa, sa), (fr, sr), (fh, sh) = pairs
            assert flat(fa[2]) == flat(sa[2]) and same(fa[0], sa[0]) and same(fa[1], sa[1]), where
            assert same_call(fr, sr) and same_call(fh, sh), where
            for fl in (fa[2], fr[3], fh[3]):
                assert [(n, u) for n, u in raised(fl) if not n.startswith("checked")] == [("key", row)], (where, raised(fl))
                assert int(np.asarray(fl["key"]).reshape(-1)[row]) == SUM, where
                # the residue identity of the inner product holds on the key as it is
                mac = fl["checked"]["mac"] if "mac" in fl["checked"] else fl["checked"]["keyswitch"]["mac"]
                assert not np.asarray(mac).any(), where

        for row, j in c.key_words():
            flip(eng, c.dk, row * N + j, 3)
            try:
                pairs = all_calls(c.key_seal)
            finally:
                flip(eng, c.dk, row * N + j, 3)
            check_all(pairs, row, (row, j))
        # a changed seal word
        row = c.key_row(c.dnum - 1, 1, c.L)
        s = c.key_seal.download().copy().reshape(c.rows, 2)
        s[row, 1] ^= np.uint64(1 << 33)
        check_all(all_calls(eng.upload(s)), row, "seal word")
        # the call after it is clean
        assert all(raised(f[-1]) == [] for f, _ in all_calls(c.key_seal))
        assert c.unchanged()
    eng.check()


@pytest.mark.parametrize("name,tp", FUSED + BANDS)
def test_a_fault_on_the_multiplying_load_is_seen_by_the_fused_calls_only(F, eng, cases, name, tp):
    c = cases(name)
    ks, ab, N = c.ks, c.ab, c.N
    with plain_modulus(ks, tp):
        rk = dict(seals=c.seals[:2], key_seal=c.key_seal)
        hk = dict(seals=c.seals, key_seal=c.key_seal, rescale=True)
        calls = {
            "apply": (lambda: swept_apply(c, tp), lambda: ks.apply_sealed(c.d[0], c.dk, ab, key_seal=c.key_seal)),
            "rotate": (lambda: ks.rotate_sealed(c.d[0], c.d[1], GALOIS, c.dk, ab, **rk), lambda: ks.rotate_sealed_fused(c.d[0], c.d[1], GALOIS, c.dk, ab, **rk)),
            "hmult": (lambda: ks.hmult_sealed_fused(*c.d, c.dk, ab, **hk), lambda: ks.hmult_sealed_fused_key(*c.d, c.dk, ab, **hk)),
        }
        words = c.key_words()
        # above two chunks per row: the apply call's hook on both sides of the last chunk edge as well
        hooked = list(zip(calls.items(), (words[4], words[2], words[3]))) + [(("apply", calls["apply"]), w) for w in words[5:]]
        for (what, (swept, fused)), (row, j) in hooked:
            clean = fused()
            assert raised(clean[-1]) == []
            eng.inject_fault_keyswitch_sealed(row, j, 3)
            # the sweep-based call does not run the sealed inner product: it leaves the hook armed, and sees nothing
            got = swept()
            assert raised(got[-1]) == [] and same(got[0], clean[0]) and same(got[1], clean[1]), what
            got = fused()
            fl = got[-1]
            assert raised(fl) == [("key", row)] and int(np.asarray(fl["key"]).reshape(-1)[row]) == SUM, (what, raised(fl))
            mac = fl["checked"]["mac"] if "mac" in fl["checked"] else fl["checked"]["keyswitch"]["mac"]
            assert not np.asarray(mac).any(), what
            assert not (same(got[0], clean[0]) and same(got[1], clean[1])), what      # the product is that of the word as loaded
            assert c.unchanged(), what                                                  # memory is clean
            again = fused()                                                           # one shot
            assert raised(again[-1]) == [] and same(again[0], clean[0]) and same(again[1], clean[1]), what
        # out of the window on the load: both bits on the key row, and that half of the inner product cannot be checked
        row = c.key_row(0, 1, 1)
        eng.inject_fault_keyswitch_sealed(row, 1, 63)
        fl = ks.apply_sealed(c.d[0], c.dk, ab, key_seal=c.key_seal)[2]
        assert [(n, u, int(np.asarray(fl["key"]).reshape(-1)[u])) for n, u in raised(fl) if n == "key"] == [("key", row, SUM | RANGE)]
        assert fl["checked"]["mac"].tolist()[1][1] == 4 and not fl["checked"]["mac"][0].any()
        # without a stored seal nothing is compared, but the window is still checked
        eng.inject_fault_keyswitch_sealed(row, 1, 63)
        fl = ks.apply_sealed(c.d[0], c.dk, ab)[2]
        assert [(n, u, int(np.asarray(fl["key"]).reshape(-1)[u])) for n, u in raised(fl) if n == "key"] == [("key", row, RANGE)]
        eng.inject_fault_keyswitch_sealed(row, 1, 3)
        assert raised(ks.apply_sealed(c.d[0], c.dk, ab)[2]) == []
    eng.check()


@pytest.mark.parametrize("name,tp", PARAMS)
def test_the_steps_hooks_fire_in_their_own_step(F, eng, cases, name, tp):
    from fhe_reliability_gpu_amd._lib import check, lib
    c = cases(name)
    ks, ab, L, N = c.ks, c.ab, c.L, c.N
    arm_ks = lib.fhe_ctx_inject_fault_bgv_keyswitch if tp else lib.fhe_ctx_inject_fault_keyswitch
    arm_rs = lib.fhe_ctx_inject_fault_bgv_mod_switch if tp else lib.fhe_ctx_inject_fault_rescale
    with plain_modulus(ks, tp):
        check(arm_ks(eng._h, 7, 2, 1, 3, 30))                # the tail, the word before its window check, unit 1
        assert raised(ks.apply_sealed(c.d[0], c.dk, ab, key_seal=c.key_seal)[2]) == [("checked.tail", 1)]
        check(arm_ks(eng._h, 3, 2, c.M + 1, 3, 30))          # the sealed inner product itself, half 1, row 1: its residue word
        assert raised(ks.apply_sealed(c.d[0], c.dk, ab, key_seal=c.key_seal)[2]) == [("checked.mac", c.M + 1)]
        check(arm_ks(eng._h, 3, 2, 0, 5, 30))
        fl = ks.rotate_sealed_fused(c.d[0], c.d[1], GALOIS, c.dk, ab, seals=c.seals[:2], key_seal=c.key_seal)[3]
        assert raised(fl) == [("checked.mac", 0)], raised(fl)
        kw = dict(seals=c.seals, key_seal=c.key_seal, rescale=True)
        check(arm_ks(eng._h, 7, 2, 1, 3, 30))
        assert raised(ks.hmult_sealed_fused_key(*c.d, c.dk, ab, **kw)[3]) == [("checked.keyswitch.tail", 1)]
        check(arm_rs(eng._h, 3, 2, 1, 3, 30))                # (c - delta) / q_last, the word before its window check, unit 1
        got = raised(ks.hmult_sealed_fused_key(*c.d, c.dk, ab, **kw)[3])
        assert len(got) == 1 and got[0][0].startswith("checked.rescale.") and got[0][1] == 1, got
        check(lib.fhe_ctx_inject_fault_pointwise(eng._h, 2, (L - 1) * N + 5, 3))
        assert raised(ks.hmult_sealed_fused_key(*c.d, c.dk, ab, **kw)[3]) == [("checked.tensor", 3 * (L - 1) + 1)]
        assert raised(ks.hmult_sealed_fused_key(*c.d, c.dk, ab, **kw)[3]) == []
    eng.check()


def raw_apply(eng, c, flags, abft="own", evk=None, out1=None, o=None):
    from fhe_reliability_gpu_amd._lib import lib
    o0, o1 = o
    return lib.fhe_keyswitch_apply_sealed(eng._h, c.ks._h, o0.ptr, o1.ptr if out1 is None else out1, c.d[0].ptr, c.dk.ptr if evk is None else evk, None, None,
                                          c.ab._h if abft == "own" else abft, c.key_seal.ptr, flags, None)


def test_above_the_cap_an_armed_hook_is_refused_and_nothing_is_launched(F, eng, cases):
    from fhe_reliability_gpu_amd._lib import lib
    c = cases("D")
    ks, ab, N, L = c.ks, c.ab, c.N, c.L
    assert not ks.apply_sealed_layout()["fused"]
    total = ks.apply_sealed_layout()["total"]
    n_words = (total + 1) // 2 + 64
    o = (eng.alloc(L * N), eng.alloc(L * N))
    fl = eng.upload(np.full(n_words, GARBAGE, dtype=np.uint64))
    eng.inject_fault_keyswitch_sealed(0, 0, 3)
    assert raw_apply(eng, c, fl.ptr, o=o) == INVALID and "outside the call" in lib.fhe_last_error().decode()
    assert (fl.download() == GARBAGE).all()
    assert raw_apply(eng, c, fl.ptr, o=o) == 0 and not fl.download().view(np.uint32)[:total].any()      # the hook is gone
    for call in (lambda: ks.rotate_sealed_fused(c.d[0], c.d[1], GALOIS, c.dk, ab, seals=c.seals[:2], key_seal=c.key_seal),
                 lambda: ks.hmult_sealed_fused_key(*c.d, c.dk, ab, seals=c.seals, key_seal=c.key_seal)):
        eng.inject_fault_keyswitch_sealed(1, 1, 3)
        with pytest.raises(F.FheError, match="outside the call"):
            call()
        assert raised(call()[3]) == []
    eng.check()


def test_refusals_launch_nothing_and_take_the_hooks(F, eng, cases):
    from fhe_reliability_gpu_amd._lib import check, lib
    c = cases("A")
    ks, N, L = c.ks, c.N, c.L
    total = ks.apply_sealed_layout()["total"]
    n_words = (total + 1) // 2 + 64
    o = (eng.alloc(L * N), eng.alloc(L * N))

    def refused(status, why, **kw):
        fl = eng.upload(np.full(n_words, GARBAGE, dtype=np.uint64))
        assert raw_apply(eng, c, fl.ptr, o=o, **kw) == status and why in lib.fhe_last_error().decode(), (why, lib.fhe_last_error())
        assert (fl.download() == GARBAGE).all()      # nothing launched, not even the clearing of the flags

    fl = eng.upload(np.full(n_words, GARBAGE, dtype=np.uint64))
    clean = lambda: raw_apply(eng, c, fl.ptr, o=o) == 0 and not fl.download().view(np.uint32)[:total].any()
    assert clean()
    refused(INVALID, "null", abft=None)
    refused(INVALID, "16-byte", evk=c.dk.ptr.value + 8)
    refused(INVALID, "distinct", out1=o[0].ptr)
    assert raw_apply(eng, c, None, o=o) == INVALID and "null" in lib.fhe_last_error().decode()
    # a hook outside the call: refused, and gone afterwards
    for bad in ((c.rows, 0, 3), (0, N, 3)):
        eng.inject_fault_keyswitch_sealed(*bad)
        refused(INVALID, "outside the call")
        assert clean()
    check(lib.fhe_ctx_inject_fault_keyswitch(eng._h, 3, 2, 2 * c.M, 0, 3))      # the checked key switch's own hook, outside stage 3
    refused(INVALID, "outside the call")
    assert clean()
    # the setter
    for bad in ((0, -1, 0), (0, 0, 64), (0, 0, -1)):
        assert lib.fhe_ctx_inject_fault_keyswitch_sealed(eng._h, *bad) == INVALID
    eng.inject_fault_keyswitch_sealed(1, 0, 3)
    eng.inject_fault_keyswitch_sealed(-1)                      # disarmed
    assert clean()
    # a refused call takes the hook with it
    for kw in (dict(abft=None), dict(evk=c.dk.ptr.value + 8), dict(out1=o[0].ptr)):
        eng.inject_fault_keyswitch_sealed(1, 0, 3)
        refused(INVALID, "", **kw)
        assert clean()
    eng.inject_fault_keyswitch_sealed(1, 0, 3)
    assert raw_apply(eng, c, None, o=o) == INVALID
    assert clean()
    # the fused composites refuse a hook outside the call as well, before any sweep, and take it
    n_rot = (ks.rotate_sealed_layout()["total"] + 1) // 2 + 64
    flr = eng.upload(np.full(n_rot, GARBAGE, dtype=np.uint64))
    sin = (C.c_void_p * 2)(c.seals[0].ptr, c.seals[1].ptr)
    rot = lambda: lib.fhe_rotate_sealed_fused(eng._h, ks._h, o[0].ptr, o[1].ptr, c.d[0].ptr, c.d[1].ptr, GALOIS, c.dk.ptr, c.ab._h, sin, c.key_seal.ptr, None,
                                              flr.ptr, None)
    eng.inject_fault_keyswitch_sealed(c.rows, 0, 3)
    assert rot() == INVALID and "outside the call" in lib.fhe_last_error().decode()
    assert (flr.download() == GARBAGE).all()
    assert rot() == 0 and not flr.download().view(np.uint32)[:ks.rotate_sealed_layout()["total"]].any()
    eng.check()
