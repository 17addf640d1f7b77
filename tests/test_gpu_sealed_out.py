"""The sealed composites whose last launch writes the outputs' seals from the registers it stores (hmult_sealed_out,
rotate_sealed_out), on the GPU: words and whole flag buffers are those of hmult_sealed_fused_key and rotate_sealed_in, the output
seals are NttTables.seal's of the outputs, and a fault after the digest -- which the sweep-based siblings cannot even be given --
leaves the returned seal that of the fault-free output, so that the next verification raises exactly that row.

Plans (logn, L, K, dnum) as test_gpu_ntt_sealed.py: A (10, 4, 2, 2), B (13, 3, 1, 3) with a 61-bit prime among 50-bit ones, C (14,
6, 2, 3), two chunks per row.  Each without and with plain modulus 65537."""
import numpy as np
import pytest

from helpers.sealed_case import SealedCase, case_cache, flat, plain_modulus, plans, same

pytestmark = pytest.mark.gpu

INVALID = 1
LOAD, STORE = 0, 1
GARBAGE = 0x5A5A5A5A5A5A5A5A
PLANS = plans("ABC")
PARAMS = [(name, tp) for name in PLANS for tp in (0, 65537)]
GALOIS = 5
CHUNK = 8192


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


class Case(SealedCase):
    """a plan, its detector, seeded operands and key on the device, and their seals"""

    def __init__(self, F, eng, name):
        logn, _, _, dnum, _ = PLANS[name]
        super().__init__(F, eng, PLANS[name], seed=419 + logn + dnum, margin=16)
        self.edge = CHUNK if self.N > CHUNK else self.N // 2


@pytest.fixture(scope="module")
def cases(F, eng):
    return case_cache(lambda name: Case(F, eng, name))


def any_raised(d):
    return any(any(v) for _, v in flat(d))


def calls(c, which):
    """(the _out call, its sweep-based sibling, rows per output) of hmult with rescale, hmult without, or the rotation"""
    ks, ab = c.ks, c.ab
    if which == "rotate":
        kw = dict(seals=c.seals[:2], key_seal=c.key_seal)
        return (lambda: ks.rotate_sealed_out(c.d[0], c.d[1], GALOIS, c.dk, ab, **kw), lambda: ks.rotate_sealed_in(c.d[0], c.d[1], GALOIS, c.dk, ab, **kw), c.L)
    rescale = which == "hmult_rescale"
    kw = dict(seals=c.seals, key_seal=c.key_seal, rescale=rescale)
    return (lambda: ks.hmult_sealed_out(*c.d, c.dk, ab, **kw), lambda: ks.hmult_sealed_fused_key(*c.d, c.dk, ab, **kw), c.L - 1 if rescale else c.L)


WHICH = ("hmult_rescale", "hmult", "rotate")


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("name,tp", PARAMS)
def test_words_flags_and_seals_are_the_siblings(F, eng, cases, name, tp, which):
    c = cases(name)
    with plain_modulus(c.ks, tp):
        out, sib, limbs = calls(c, which)
        o0, o1, so, fl = out()
        r0, r1, rs, rf = sib()
        assert not any_raised(fl)
        assert same(o0, r0) and same(o1, r1)
        assert flat(fl) == flat(rf)
        assert same(so[0], rs[0]) and same(so[1], rs[1])
        assert same(so[0], c.t.seal(o0, limbs=limbs)) and same(so[1], c.t.seal(o1, limbs=limbs))
        assert c.unchanged()
    eng.check()


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("name,tp", PARAMS)
def test_a_fault_after_the_digest_is_caught_by_the_next_verification(F, eng, cases, name, tp, which):
    c = cases(name)
    with plain_modulus(c.ks, tp):
        out, sib, limbs = calls(c, which)
        clean = out()
        for half, l, j in ((0, 1, c.edge - 1), (1, limbs - 1, c.edge)):
            eng.inject_fault_subscale_sealed(STORE, half * limbs + l, j, 3)
            # the sweep-based sibling does not run the sealed tail: it sees nothing and leaves the hook armed
            r = sib()
            assert not any_raised(r[3]) and same(r[0], clean[0]) and same(r[1], clean[1]) and same(r[2][half], clean[2][half])
            o0, o1, so, fl = out()
            assert not any_raised(fl)
            assert same(so[0], clean[2][0]) and same(so[1], clean[2][1])      # the seals of the fault-free outputs
            got, want = (o0, o1)[half].download().reshape(limbs, c.N), clean[half].download().reshape(limbs, c.N)
            assert np.argwhere(got != want).tolist() == [[l, j]] and int(got[l, j]) == int(want[l, j]) ^ 8
            assert same((o0, o1)[1 - half], clean[1 - half])
            v = [np.asarray(c.t.seal_verify(o, s, limbs=limbs)).reshape(-1) for o, s in zip((o0, o1), so)]
            assert np.flatnonzero(v[half]).tolist() == [l] and not v[1 - half].any()
            again = out()                                                     # one shot
            assert same(again[0], clean[0]) and same(again[1], clean[1])
        assert c.unchanged()
    eng.check()


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("name,tp", PARAMS[:2])
def test_hooks_that_do_not_fit_are_refused(F, eng, cases, name, tp, which):
    from fhe_reliability_gpu_amd._lib import FheError
    c = cases(name)
    with plain_modulus(c.ks, tp):
        out, sib, limbs = calls(c, which)
        clean = out()
        for args, why in (((LOAD, 0, 0, 3), "input seal step"), ((STORE, 2 * limbs, 0, 3), "outside the call"), ((STORE, 0, c.N, 3), "outside the call")):
            eng.inject_fault_subscale_sealed(*args)
            with pytest.raises(FheError, match=why):
                out()
            got = out()                                                       # the refused call took the hook
            assert not any_raised(got[3]) and same(got[0], clean[0]) and same(got[2][0], clean[2][0])
        eng.inject_fault_subscale_sealed(STORE, 0, 0, 3)
        eng.inject_fault_subscale_sealed(-1)                                  # disarmed
        assert same(out()[0], clean[0])
    eng.check()


class _Off:
    """a device array's pointer moved by 8 bytes: refused for its alignment, before anything is launched"""

    def __init__(self, d):
        import ctypes
        self.ptr = ctypes.c_void_p(d.ptr.value + 8)


@pytest.mark.parametrize("tp", (0, 65537))
def test_a_refused_composite_takes_every_hook_it_owns(F, eng, tp):
    """The sweep-based composites at each refusal kind -- scope, alignment, an unpaired locator, a sealed step's hit outside the call
    -- with every hook the call owns armed: the next valid call runs clean.  The smallest plan: N = 2^10, L = 3, K = 1, dnum = 3."""
    from fhe_reliability_gpu_amd._lib import FheError, check, lib
    c = SealedCase(F, eng, (10, 3, 1, 3, [50, 61, 50, 50]), seed=431, margin=16)
    ks, ab, d, h = c.ks, c.ab, c.d, eng._h
    locs, key_loc = [c.t.seal_locator(v, limbs=c.L) for v in d], ks.seal_key_locator(c.dk)
    kw = dict(seals=c.seals, key_seal=c.key_seal)

    def arm(tensor_row=1):
        check((lib.fhe_ctx_inject_fault_bgv_keyswitch if tp else lib.fhe_ctx_inject_fault_keyswitch)(h, 3, 0, 1, 5, 3))
        check((lib.fhe_ctx_inject_fault_bgv_mod_switch if tp else lib.fhe_ctx_inject_fault_rescale)(h, 1, 0, 1, 5, 3))
        check(lib.fhe_ctx_inject_fault_pointwise(h, 0, 7, 3))
        eng.inject_fault_tensor_sealed(2, tensor_row, 6, 3)
        eng.inject_fault_keyswitch_sealed(c.M + 1, 4, 3)
        eng.inject_fault_subscale_sealed(STORE, 1, 3, 3)

    def out_of_scope(call):
        eng.set_option("ntt_mode", 1)
        try:
            call()
        finally:
            eng.set_option("ntt_mode", 0)

    hm_out = lambda a0=d[0]: ks.hmult_sealed_out(a0, d[1], d[2], d[3], c.dk, ab, **kw)
    rot = lambda c0=d[0]: ks.rotate_sealed_fused(c0, d[1], GALOIS, c.dk, ab, seals=c.seals[:2], key_seal=c.key_seal)
    repair = lambda a0=d[0], l=locs: ks.hmult_sealed_repair(a0, d[1], d[2], d[3], c.dk, ab, seals=c.seals, locators=l, key_seal=c.key_seal, key_locator=key_loc)
    with plain_modulus(ks, tp):
        # (the valid call, its refusals by kind): a call's own hooks are a subset of those armed
        for valid, refusals in ((hm_out, {"two-launch": lambda: out_of_scope(hm_out), "16-byte": lambda: hm_out(_Off(d[0])), "outside the call": hm_out}),
                                (rot, {"two-launch": lambda: out_of_scope(rot), "16-byte": lambda: rot(_Off(d[0]))}),
                                (repair, {"two-launch": lambda: out_of_scope(repair), "16-byte": lambda: repair(_Off(d[0])),
                                          "together": lambda: repair(l=[locs[0], None, locs[2], locs[3]])})):
            clean = valid()
            assert not any_raised(clean[-2] if valid is repair else clean[3])
            for why, refused in refusals.items():
                arm(tensor_row=c.L if why == "outside the call" else 1)
                with pytest.raises(FheError, match=why):
                    refused()
                got = valid()      # the refused call took its hooks
                assert not any_raised(got[-2] if valid is repair else got[3]), why
                assert same(got[0], clean[0]) and same(got[1], clean[1]) and same(got[2][0], clean[2][0]) and same(got[2][1], clean[2][1])
                hm_out()           # takes what the refused call did not own
        assert c.unchanged()
    eng.check()
