"""The sealed multiply without its four operand sweeps (hmult_sealed_fused) on the GPU: the words are hmult's, the output seals
verify, and for corruptions at rest the flag buffer and the output words are hmult_sealed's, word for word.  What only the fused call
can see: a fault on the load that multiplies.

Plans (logn, L, K, dnum): (10, 4, 2, 2), (13, 3, 1, 3) with a 61-bit prime among 50-bit ones, (14, 6, 2, 3) the reference's shape;
each without and with plain modulus 65537, without and with the rescale."""
import numpy as np
import pytest

from helpers.sealed_case import SealedCase, case_cache, flat, flip, plain_modulus, plans, py_seals, raised, same

pytestmark = pytest.mark.gpu

INVALID = 1
SUM, RANGE = 1, 2
GARBAGE = 0x5A5A5A5A5A5A5A5A
PLANS = plans("ABC")
NAMES = ("a0", "a1", "b0", "b1")
PARAMS = [(name, tp, resc) for name in PLANS for tp in (0, 65537) for resc in (False, True)]


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
        super().__init__(F, eng, PLANS[name], seed=77 + PLANS[name][0], margin=16)      # bit 3 flips stay below q
        for v, s in zip(self.ops, self.seals):
            assert s.download().tolist() == py_seals(v)


@pytest.fixture(scope="module")
def cases(F, eng):
    return case_cache(lambda name: Case(F, eng, name))


@pytest.mark.parametrize("name,tp,resc", PARAMS)
def test_clean_words_are_hmults_seals_verify_and_no_flag(F, eng, cases, name, tp, resc):
    c = cases(name)
    ks, ab, L = c.ks, c.ab, c.L
    with plain_modulus(ks, tp):
        o0, o1, so, fl = ks.hmult_sealed_fused(*c.d, c.dk, ab, seals=c.seals, key_seal=c.key_seal, rescale=resc)
        assert raised(fl) == [], raised(fl)
        w0, w1 = ks.hmult(*c.d, c.dk, rescale=resc)
        assert same(o0, w0) and same(o1, w1)
        limbs = L - 1 if resc else L
        for o, s in zip((o0, o1), so):
            assert not c.t.seal_verify(o, s, limbs=limbs).any()
        assert so[0].download().tolist() == py_seals(w0.download())
        # the same structure as the sweep-based call, word for word
        ref = ks.hmult_sealed(*c.d, c.dk, ab, seals=c.seals, key_seal=c.key_seal, rescale=resc)
        assert flat(fl) == flat(ref[3]) and same(o0, ref[0]) and same(o1, ref[1])
        assert all((dv.download().reshape(-1) == v.reshape(-1)).all() for dv, v in zip(c.d + [c.dk], c.ops + [c.key]))
    eng.check()


@pytest.mark.parametrize("name,tp,resc", PARAMS)
def test_corruptions_at_rest_give_the_sweep_based_calls_flags_and_words(F, eng, cases, name, tp, resc):
    c = cases(name)
    ks, ab, L, N, M = c.ks, c.ab, c.L, c.N, c.M
    key_row = (1 * 2 + 1) * M + (M - 1)                      # digit 1, half 1, the last special limb
    chunk_edge = (1 << 13) if c.logn > 13 else N // 2
    # (what is raised, device array, word index)
    targets = [("a0", c.d[0], (L - 1) * N + N - 1), ("a1", c.d[1], 0), ("b0", c.d[2], 1 * N + chunk_edge - 1), ("b1", c.d[3], (L - 2) * N + chunk_edge),
               ("key", c.dk, key_row * N + 9)]
    with plain_modulus(ks, tp):
        kw = dict(key_seal=c.key_seal, rescale=resc)
        for what, dev, idx in targets:
            flip(eng, dev, idx, 3)
            try:
                fused = ks.hmult_sealed_fused(*c.d, c.dk, ab, seals=c.seals, **kw)
                swept = ks.hmult_sealed(*c.d, c.dk, ab, seals=c.seals, **kw)
            finally:
                flip(eng, dev, idx, 3)
            assert flat(fused[3]) == flat(swept[3]), what
            assert [(n, u) for n, u in raised(fused[3]) if not n.startswith("checked")] == [(what, idx // N)], (what, raised(fused[3]))
            assert int(np.asarray(fused[3][what]).reshape(-1)[idx // N]) == SUM
            assert same(fused[0], swept[0]) and same(fused[1], swept[1]), what
        # a changed seal word
        s = c.seals[2].download().copy()
        s[L - 1, 0] ^= np.uint64(1 << 33)
        seals = list(c.seals)
        seals[2] = eng.upload(s)
        fused = ks.hmult_sealed_fused(*c.d, c.dk, ab, seals=seals, **kw)
        swept = ks.hmult_sealed(*c.d, c.dk, ab, seals=seals, **kw)
        assert flat(fused[3]) == flat(swept[3]) and raised(fused[3]) == [("b0", L - 1)]
        assert same(fused[0], swept[0]) and same(fused[1], swept[1])
        assert raised(ks.hmult_sealed_fused(*c.d, c.dk, ab, seals=c.seals, **kw)[3]) == []
    eng.check()


@pytest.mark.parametrize("name,tp,resc", PARAMS)
def test_a_fault_on_the_multiplying_load_is_seen_by_the_fused_call_only(F, eng, cases, name, tp, resc):
    c = cases(name)
    ks, ab, L, N = c.ks, c.ab, c.L, c.N
    with plain_modulus(ks, tp):
        kw = dict(seals=c.seals, key_seal=c.key_seal, rescale=resc)
        clean = ks.hmult_sealed_fused(*c.d, c.dk, ab, **kw)
        for o, row, j in ((0, 0, N - 1), (3, L - 1, N // 2)):
            eng.inject_fault_tensor_sealed(o, row, j, 3)
            # the sweep-based call does not run the sealed tensor step: it leaves the hook armed, and sees nothing
            swept = ks.hmult_sealed(*c.d, c.dk, ab, **kw)
            assert raised(swept[3]) == [] and same(swept[0], clean[0]) and same(swept[1], clean[1])
            fused = ks.hmult_sealed_fused(*c.d, c.dk, ab, **kw)
            assert raised(fused[3]) == [(NAMES[o], row)] and int(fused[3][NAMES[o]][row]) == SUM, raised(fused[3])
            assert not (same(fused[0], clean[0]) and same(fused[1], clean[1]))      # the product is that of the word as loaded
            assert all((dv.download().reshape(-1) == v.reshape(-1)).all() for dv, v in zip(c.d, c.ops))      # memory is clean
            again = ks.hmult_sealed_fused(*c.d, c.dk, ab, **kw)                      # one shot
            assert raised(again[3]) == [] and same(again[0], clean[0]) and same(again[1], clean[1])
    eng.check()


@pytest.mark.parametrize("name,tp,resc", PARAMS)
def test_the_steps_hooks_fire_in_their_own_step(F, eng, cases, name, tp, resc):
    from fhe_reliability_gpu_amd._lib import check, lib
    c = cases(name)
    ks, ab, L, N = c.ks, c.ab, c.L, c.N
    arm_ks = lib.fhe_ctx_inject_fault_bgv_keyswitch if tp else lib.fhe_ctx_inject_fault_keyswitch
    arm_rs = lib.fhe_ctx_inject_fault_bgv_mod_switch if tp else lib.fhe_ctx_inject_fault_rescale
    with plain_modulus(ks, tp):
        kw = dict(seals=c.seals, key_seal=c.key_seal, rescale=resc)
        check(arm_ks(eng._h, 7, 2, 1, 3, 30))                # the tail, the word before its window check, unit 1
        fl = ks.hmult_sealed_fused(*c.d, c.dk, ab, **kw)[3]
        assert raised(fl) == [("checked.keyswitch.tail", 1)], raised(fl)
        if resc:
            check(arm_rs(eng._h, 3, 2, 1, 3, 30))            # (c - delta) / q_last, the word before its window check, unit 1
            got = raised(ks.hmult_sealed_fused(*c.d, c.dk, ab, **kw)[3])
            assert len(got) == 1 and got[0][0].startswith("checked.rescale.") and got[0][1] == 1, got
        check(lib.fhe_ctx_inject_fault_pointwise(eng._h, 2, (L - 1) * N + 5, 3))
        fl = ks.hmult_sealed_fused(*c.d, c.dk, ab, **kw)[3]
        assert raised(fl) == [("checked.tensor", 3 * (L - 1) + 1)], raised(fl)
        assert raised(ks.hmult_sealed_fused(*c.d, c.dk, ab, **kw)[3]) == []
    eng.check()


def test_refusals_launch_nothing_and_take_the_hooks(F, eng, cases):
    from fhe_reliability_gpu_amd._lib import lib, vp
    c = cases("A")
    ks, ab, N, L = c.ks, c.ab, c.N, c.L
    o0, o1 = eng.alloc(L * N), eng.alloc(L * N)
    n_words = (ks.hmult_sealed_layout(True)["total"] + 1) // 2 + 64
    sin = (vp * 4)(*[s.ptr for s in c.seals])
    ptr = lambda x, off=0: x.ptr.value + off

    def call(flags, ops=None, abft=ab._h, out1=None):
        ops = [ptr(x) for x in c.d] if ops is None else ops
        return lib.fhe_hmult_sealed_fused(eng._h, ks._h, o0.ptr, o1.ptr if out1 is None else out1, ops[0], ops[1], ops[2], ops[3], c.dk.ptr, 1, abft, sin,
                                          c.key_seal.ptr, None, flags, None)

    def refused(status, why, **kw):
        fl = eng.upload(np.full(n_words, GARBAGE, dtype=np.uint64))
        assert call(fl.ptr, **kw) == status and why in lib.fhe_last_error().decode(), (why, lib.fhe_last_error())
        assert (fl.download() == GARBAGE).all()      # nothing launched, not even a verification

    total = ks.hmult_sealed_layout(True)["total"]
    fl = eng.upload(np.full(n_words, GARBAGE, dtype=np.uint64))
    assert call(fl.ptr) == 0 and not fl.download().view(np.uint32)[:total].any()
    refused(INVALID, "null", abft=None)
    ops = [ptr(x) for x in c.d]
    ops[2] += 8
    refused(INVALID, "16-byte", ops=ops)
    ops[2] = None
    refused(INVALID, "null", ops=ops)
    refused(INVALID, "distinct", out1=o0.ptr)
    assert call(None) == INVALID
    # a hook outside the call: refused before the key's sweep, and gone afterwards
    for bad in ((1, L, 0, 3), (2, 0, N, 3)):
        eng.inject_fault_tensor_sealed(*bad)
        refused(INVALID, "outside the call")
        assert call(fl.ptr) == 0 and not fl.download().view(np.uint32)[:total].any()
    # a refused call takes the hook with it
    eng.inject_fault_tensor_sealed(0, 0, 0, 3)
    refused(INVALID, "null", abft=None)
    assert call(fl.ptr) == 0 and not fl.download().view(np.uint32)[:total].any()
    eng.check()
