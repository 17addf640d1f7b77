"""The BGV forms of the stage-by-stage checked key switch, mod switch and multiply, and the checked scalar multiply they are made
with, on the GPU: clean calls return the oracle's and the unchecked calls' words bit for bit on a plan with a plain modulus, with
every flag zero from a garbage-filled buffer; one armed bit flip at (stage, unit) raises exactly that flag word and no other,
changes the outputs and leaves the next call clean; the scope limits are error statuses.

Two plans: A = 2^10, L 4, K 2, dnum 2, all 50-bit (one-launch transforms); B = 2^13, L 3, K 1, dnum 3 with a 61-bit prime among
50-bit ones -- the smallest two-launch size, one-limb conversions on both conversion stages, the integer path beside the FP64 one.

The multiply's oracle is tensor_ref -> keyswitch_ref(plain_modulus=t) -> rescale_ref(plain_modulus=t): oracle.keyswitch_ref.hmult_ref
hands its plain modulus to the rescale only and relinearises in the CKKS form, which is not what fhe_hmult computes on a BGV plan
(the test asserts that difference once, so that the choice of reference is on record)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
RESIDUE, RANGE, OPERAND = 1, 2, 4
PRODUCT, QUOTIENT, RESULT, SUM = 0, 1, 2, 3
PLANS = {"A": (10, 4, 2, 2, [50] * 6), "B": (13, 3, 1, 3, [50, 61, 50, 50])}
GARBAGE = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


class Case:
    """a plan, its detector, seeded operands on the host and on the device"""

    def __init__(self, F, eng, name):
        self.logn, self.L, self.K, self.dnum, bits = PLANS[name]
        self.N, self.M, self.R = 1 << self.logn, self.L + self.K, self.L - 1
        self.qs = F.create_moduli(self.N, bits)
        self.t = eng.tables(self.logn, self.qs)
        self.ks, self.ab = F.KeySwitch(eng, self.t, self.L, self.K, self.dnum), F.Abft(eng, self.t)
        rng = np.random.default_rng(self.logn)
        poly = lambda: np.stack([rng.integers(0, q, self.N, dtype=np.uint64) for q in self.qs[:self.L]])
        self.ops = [poly() for _ in range(4)]
        self.key = np.stack([np.stack([np.stack([rng.integers(0, q, self.N, dtype=np.uint64) for q in self.qs]) for _ in range(2)])
                             for _ in range(self.dnum)])
        self.d = [eng.upload(v) for v in self.ops]
        self.dk = eng.upload(self.key)
        self.dc3 = eng.upload(np.stack(self.ops[:3]))


@pytest.fixture(scope="module")
def cases(F, eng):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(F, eng, name)
        return made[name]
    return get


class plain_modulus:
    def __init__(self, ks, t):
        self.ks, self.t = ks, t

    def __enter__(self):
        self.ks.set_plain_modulus(self.t)

    def __exit__(self, *exc):
        self.ks.set_plain_modulus(0)


def _raised(flags):
    """[(block, stage, flat unit)] of every raised word of a key switch's, a mod switch's or a multiply's flags"""
    out = []
    if "tensor" in flags:
        out += [("tensor", "tensor", int(u)) for u in np.flatnonzero(flags["tensor"].reshape(-1))]
        blocks = [("keyswitch", flags["keyswitch"])] + ([("rescale", flags["rescale"])] if flags["rescale"] is not None else [])
    else:
        blocks = [("", flags)]
    for block, d in blocks:
        for name, f in d.items():
            out += [(block, name, int(u)) for u in np.flatnonzero(f.reshape(-1))]
    return out


def _eq(got, want, what):
    for g, w in zip(got, want):
        g = g.download() if hasattr(g, "download") else g
        w = w.download() if hasattr(w, "download") else w
        assert (g.reshape(-1) == np.asarray(w).reshape(-1)).all(), what


def _sigma_ntt(x, k, qs, logn):
    """sigma_k of an NTT-domain polynomial, through the coefficient domain (as oracle.keyswitch_ref.rotate_ref does)"""
    from oracle import cport as O
    from oracle.keyswitch_ref import galois_coeff
    rps = np.stack([O.root_powers(q, logn) for q in qs])
    co = O.nwt_inverse_batch(np.asarray(x, dtype=np.uint64), qs, rps)
    return O.nwt_forward_batch(np.stack([galois_coeff(co[l], k, qs[l]) for l in range(len(qs))]), qs, rps)


@pytest.mark.parametrize("name,tp", [("A", 65537), ("A", 786433), ("B", 786433), ("B", 65537)])
def test_clean_calls_return_the_oracles_and_the_unchecked_words_and_no_flag(F, eng, cases, name, tp):
    from oracle.keyswitch_ref import hmult_ref, keyswitch_ref, rescale_ref, tensor_ref
    c = cases(name)
    ks, ab, qs, L, K, dnum, logn, R = c.ks, c.ab, c.qs, c.L, c.K, c.dnum, c.logn, c.R
    a0, a1, b0, b1 = c.ops
    oracle = name == "A" or tp == 786433      # the CPU oracle at 2^13 once
    # the layouts: the CKKS-form words first, at the offsets of the existing layout functions
    kl, bl = ks.checked_layout(), ks.bgv_checked_layout()
    assert all(bl[s] == kl[s] for s in ks.CHECKED_STAGES)
    assert bl["scale_special"] == (kl["total"], (2, K)) and bl["scale_conv"] == (kl["total"] + 2 * K, (2, L)) and bl["total"] == kl["total"] + 2 * (K + L)
    for n in (1, 2, 3):
        rl, ml = ks.rescale_checked_layout(n), ks.bgv_mod_switch_checked_layout(n)
        assert all(ml[s] == rl[s] for s in ks.RESCALE_CHECKED_STAGES)
        assert ml["scale_last"] == (rl["total"], (n,)) and ml["scale_delta"] == (rl["total"] + n, (n, R)) and ml["total"] == rl["total"] + n * L
    for resc in (True, False):
        hl = ks.bgv_hmult_checked_layout(resc)
        want_rs = 3 * L + bl["total"]
        assert hl == {"tensor": 0, "keyswitch": 3 * L, "rescale": want_rs, "total": want_rs + (ks.bgv_mod_switch_checked_layout(2)["total"] if resc else 0)}
    gal = 5
    with plain_modulus(ks, tp):
        # ---- key switch, relinearisation, rotation
        got = {}
        got["apply"] = ks.bgv_apply_checked(c.d[0], c.dk, ab)
        got["relin"] = ks.bgv_relinearize_checked(c.d[1], c.d[2], c.d[0], c.dk, ab)
        got["rotate"] = ks.bgv_rotate_checked(c.d[0], c.d[1], gal, c.dk, ab)
        for what, (o0, o1, fl) in got.items():
            assert sorted(fl) == sorted(ks.BGV_CHECKED_STAGES) and _raised(fl) == [], what
        for fused in (0, 1):
            eng.set_option("ks_fused", fused)
            try:
                _eq(got["apply"][:2], ks.apply(c.d[0], c.dk), f"apply, ks_fused {fused}")
                _eq(got["relin"][:2], ks.relinearize(c.d[1], c.d[2], c.d[0], c.dk), f"relinearize, ks_fused {fused}")
                _eq(got["rotate"][:2], ks.rotate(c.d[0], c.d[1], gal, c.dk), f"rotate, ks_fused {fused}")
            finally:
                eng.set_option("ks_fused", -1)
        if oracle:
            _eq(got["apply"][:2], keyswitch_ref(a0, c.key, qs, L, K, dnum, logn, plain_modulus=tp), "apply against the oracle")
            _eq(got["relin"][:2], keyswitch_ref(a0, c.key, qs, L, K, dnum, logn, add0=a1, add1=b0, plain_modulus=tp), "relinearize against the oracle")
            s0, s1 = _sigma_ntt(a0, gal, qs[:L], logn), _sigma_ntt(a1, gal, qs[:L], logn)
            _eq(got["rotate"][:2], keyswitch_ref(s1, c.key, qs, L, K, dnum, logn, add0=s0, plain_modulus=tp), "rotate against the oracle")
        # ---- mod switch
        for n in (1, 2, 3):
            o, fl = ks.bgv_mod_switch_checked(c.dc3, ab, n_parts=n)
            assert sorted(fl) == sorted(ks.BGV_MOD_SWITCH_CHECKED_STAGES) and _raised(fl) == [], n
            _eq([o], [ks.rescale(c.dc3, n_parts=n)], f"mod switch, {n} parts")
            if oracle:
                _eq([o], [rescale_ref(np.stack(c.ops[:3])[:n], qs, L, logn, plain_modulus=tp)], f"mod switch against the oracle, {n} parts")
        # ---- multiply
        for resc in (True, False):
            o0, o1, fl = ks.bgv_hmult_checked(*c.d, c.dk, ab, rescale=resc)
            assert (fl["rescale"] is None) == (not resc) and _raised(fl) == [], resc
            for fused in (0, 1):
                eng.set_option("hmult_fused_rescale", fused)
                try:
                    _eq((o0, o1), ks.hmult(*c.d, c.dk, rescale=resc), f"hmult, rescale {resc}, hmult_fused_rescale {fused}")
                finally:
                    eng.set_option("hmult_fused_rescale", 1)
            if oracle:
                d0, d1, d2 = tensor_ref(a0, a1, b0, b1, qs)
                w = keyswitch_ref(d2, c.key, qs, L, K, dnum, logn, add0=d0, add1=d1, plain_modulus=tp)
                if resc:
                    w = rescale_ref(list(w), qs, L, logn, plain_modulus=tp)
                _eq((o0, o1), w, f"hmult against the oracle, rescale {resc}")
                if name == "A" and tp == 65537:
                    # hmult_ref relinearises in the CKKS form whatever its plain modulus: not the BGV multiply
                    h = hmult_ref(a0, a1, b0, b1, c.key, qs, L, K, dnum, logn, rescale=resc, plain_modulus=tp)
                    assert (np.asarray(h[0]) != np.asarray(w[0])).any()
        # inputs untouched
        _eq(c.d, c.ops, "operands changed")
        _eq([c.dk], [c.key], "key changed")
    eng.check()


def _ks_cases(c):
    """(stage, point, unit, bit) for every stage of the BGV key switch on plan B (one-limb digits, K = 1: no point 3 on stages 1, 5)"""
    L, K, M = c.L, c.K, c.M
    return [(0, 0, L - 1, 30), (1, RESULT, 1, 30), (2, 0, 1, 30), (3, PRODUCT, M + 1, 30), (4, 0, K, 30), (5, RESULT, 2 * (K + L) - 1, 30),
            (6, 0, 2 * L - 1, 30), (7, SUM, L + 1, 30),
            (9, PRODUCT, 0, 30), (9, QUOTIENT, 2 * K - 1, 21), (9, RESULT, K, 30),
            (10, PRODUCT, 2 * L - 1, 30), (10, QUOTIENT, 1, 21), (10, RESULT, L, 30)]


def _ms_cases(c, n):
    R = c.R
    return [(0, 0, n - 1, 30), (1, RESULT, n * R - 1, 30), (2, 0, (n - 1) * R, 30), (3, PRODUCT, R - 1, 30),
            (4, PRODUCT, 0, 30), (4, QUOTIENT, n - 1, 21), (4, RESULT, n - 1, 30),
            (5, PRODUCT, n * R - 1, 30), (5, QUOTIENT, 0, 21), (5, RESULT, (n - 1) * R + 1, 30)]


def test_one_flip_in_the_key_switch_raises_exactly_its_own_word(F, eng, cases):
    from fhe_reliability_gpu_amd._lib import check, lib
    c = cases("B")
    ks, ab, N = c.ks, c.ab, c.N
    names = ks.BGV_CHECKED_STAGES
    name_of = {s: names[s] for s in range(8)}
    name_of.update({9: names[8], 10: names[9]})
    with plain_modulus(ks, 786433):
        run = lambda: ks.bgv_relinearize_checked(c.d[1], c.d[2], c.d[0], c.dk, ab)
        o0, o1, fl = run()
        assert _raised(fl) == []
        want = o0.download(), o1.download()
        for i, (stage, point, unit, bit) in enumerate(_ks_cases(c)):
            coeff = (0, N // 2 + 7, N - 1)[i % 3]
            check(lib.fhe_ctx_inject_fault_bgv_keyswitch(eng._h, stage, point, unit, coeff, bit))
            o0, o1, fl = run()
            assert _raised(fl) == [("", name_of[stage], unit)], f"stage {stage} point {point} unit {unit}: raised {_raised(fl)}"
            assert (o0.download() != want[0]).any() or (o1.download() != want[1]).any(), f"stage {stage} unit {unit}: outputs unchanged"
            o0, o1, fl = run()      # one shot
            assert _raised(fl) == []
            _eq((o0, o1), want, f"after stage {stage}")
        # point 3 of the scalar stages: refused, nothing launched (the flag buffer keeps its pattern), nothing left armed
        lay = ks.bgv_checked_layout()
        o0, o1 = eng.alloc(c.L * N), eng.alloc(c.L * N)
        for stage in (9, 10):
            flb = eng.upload(np.full((lay["total"] + 1) // 2, GARBAGE, dtype=np.uint64))
            check(lib.fhe_ctx_inject_fault_bgv_keyswitch(eng._h, stage, SUM, 0, 0, 30))
            assert lib.fhe_bgv_keyswitch_apply_checked(eng._h, ks._h, o0.ptr, o1.ptr, c.d[0].ptr, c.dk.ptr, None, None, ab._h, flb.ptr, None) == UNSUPPORTED
            assert (flb.download() == GARBAGE).all()
            assert _raised(run()[2]) == []
        # a unit outside the stage
        check(lib.fhe_ctx_inject_fault_bgv_keyswitch(eng._h, 9, RESULT, 2 * c.K, 0, 30))
        assert lib.fhe_bgv_keyswitch_apply_checked(eng._h, ks._h, o0.ptr, o1.ptr, c.d[0].ptr, c.dk.ptr, None, None, ab._h, flb.ptr, None) == INVALID
    eng.check()


def test_one_flip_in_the_mod_switch_raises_exactly_its_own_word(F, eng, cases):
    from fhe_reliability_gpu_amd._lib import check, lib
    c = cases("B")
    ks, ab, N, R = c.ks, c.ab, c.N, c.R
    names = ks.BGV_MOD_SWITCH_CHECKED_STAGES
    with plain_modulus(ks, 65537):
        for n in (3, 1):
            dc = eng.upload(np.stack(c.ops[:3])[:n])
            o, fl = ks.bgv_mod_switch_checked(dc, ab, n_parts=n)
            assert _raised(fl) == []
            want = o.download()
            for i, (stage, point, unit, bit) in enumerate(_ms_cases(c, n)):
                coeff = (N - 1, 0, N // 2 + 7)[i % 3]
                check(lib.fhe_ctx_inject_fault_bgv_mod_switch(eng._h, stage, point, unit, coeff, bit))
                o, fl = ks.bgv_mod_switch_checked(dc, ab, n_parts=n)
                assert _raised(fl) == [("", names[stage], unit)], f"{n} parts, stage {stage} point {point} unit {unit}: raised {_raised(fl)}"
                assert (o.download() != want).any(), f"stage {stage} unit {unit}: outputs unchanged"
                o, fl = ks.bgv_mod_switch_checked(dc, ab, n_parts=n)
                assert _raised(fl) == [] and (o.download() == want).all()
        lay = ks.bgv_mod_switch_checked_layout(1)
        o = eng.alloc(R * N)
        for stage in (4, 5):
            flb = eng.upload(np.full((lay["total"] + 1) // 2, GARBAGE, dtype=np.uint64))
            check(lib.fhe_ctx_inject_fault_bgv_mod_switch(eng._h, stage, SUM, 0, 0, 30))
            assert lib.fhe_bgv_mod_switch_checked(eng._h, ks._h, o.ptr, dc.ptr, 1, ab._h, flb.ptr, None) == UNSUPPORTED
            assert (flb.download() == GARBAGE).all()
            assert _raised(ks.bgv_mod_switch_checked(dc, ab, n_parts=1)[1]) == []
    eng.check()


def test_a_call_clears_exactly_its_own_flag_words(F, eng, cases):
    """the mod switch and the key switch clear the words of their layout -- the scalar stages' included -- and not one word more"""
    from fhe_reliability_gpu_amd._lib import check, lib
    c = cases("A")
    ks, ab, N, L, R = c.ks, c.ab, c.N, c.L, c.R
    pattern = GARBAGE & 0xFFFFFFFF

    def flat_flags(total, call):
        """the call on a buffer of total + 2 patterned words: (the first total words, the two behind them)"""
        flb = eng.upload(np.full(total + 2 + total % 2, pattern, dtype=np.uint32).view(np.uint64))
        check(call(flb))
        f = flb.download().view(np.uint32)
        return f[:total], f[total:total + 2]

    with plain_modulus(ks, 65537):
        for n in (1, 3):
            lay = ks.bgv_mod_switch_checked_layout(n)
            o = eng.alloc(n * R * N)
            mod_switch = lambda flb: lib.fhe_bgv_mod_switch_checked(eng._h, ks._h, o.ptr, c.dc3.ptr, n, ab._h, flb.ptr, None)
            own, behind = flat_flags(lay["total"], mod_switch)
            assert not own.any() and (behind == pattern).all(), n
        # a fault on the last unit of the last stage: the last word of the layout, and only that one
        unit = 3 * R - 1
        check(lib.fhe_ctx_inject_fault_bgv_mod_switch(eng._h, 5, RESULT, unit, N - 1, 30))
        own, behind = flat_flags(lay["total"], mod_switch)
        assert np.flatnonzero(own).tolist() == [lay["scale_delta"][0] + unit] == [lay["total"] - 1] and (behind == pattern).all()
        lay = ks.bgv_checked_layout()
        o0, o1 = eng.alloc(L * N), eng.alloc(L * N)
        own, behind = flat_flags(lay["total"], lambda flb: lib.fhe_bgv_keyswitch_apply_checked(
            eng._h, ks._h, o0.ptr, o1.ptr, c.d[0].ptr, c.dk.ptr, None, None, ab._h, flb.ptr, None))
        assert not own.any() and (behind == pattern).all()
    eng.check()


def test_each_hook_fires_in_its_own_block_of_the_multiply(F, eng, cases):
    from fhe_reliability_gpu_amd._lib import check, lib
    c = cases("B")
    ks, ab, N, L, R = c.ks, c.ab, c.N, c.L, c.R
    with plain_modulus(ks, 786433):
        run = lambda resc=True: ks.bgv_hmult_checked(*c.d, c.dk, ab, rescale=resc)
        o0, o1, fl = run()
        assert _raised(fl) == []
        want = o0.download(), o1.download()

        def expect(block, stage, unit, what):
            o0, o1, fl = run()
            assert _raised(fl) == [(block, stage, unit)], f"{what}: raised {_raised(fl)}"
            assert (o0.download() != want[0]).any() or (o1.download() != want[1]).any(), f"{what}: outputs unchanged"
            o0, o1, fl = run()
            assert _raised(fl) == []
            _eq((o0, o1), want, what)

        check(lib.fhe_ctx_inject_fault_pointwise(eng._h, SUM, 2 * N + 9, 30))
        expect("tensor", "tensor", 3 * 2 + 1, "tensor sum")
        for stage, name, point, unit in ((9, "scale_special", RESULT, 1), (10, "scale_conv", PRODUCT, L + 2), (7, "tail", SUM, 1), (4, "intt_special", 0, 0)):
            check(lib.fhe_ctx_inject_fault_bgv_keyswitch(eng._h, stage, point, unit, N // 2 + 7, 30))
            expect("keyswitch", name, unit, f"key switch stage {stage}")
        for stage, name, point, unit in ((4, "scale_last", RESULT, 1), (5, "scale_delta", PRODUCT, R + 1), (1, "reduce", RESULT, 0), (2, "ntt_delta", 0, R)):
            check(lib.fhe_ctx_inject_fault_bgv_mod_switch(eng._h, stage, point, unit, N - 1, 30))
            expect("rescale", name, unit, f"mod switch stage {stage}")
        # the offsets in the one buffer are the layout's: a raw call, flags read back flat
        lay, ml = ks.bgv_hmult_checked_layout(True), ks.bgv_mod_switch_checked_layout(2)
        p0, p1 = eng.alloc(R * N), eng.alloc(R * N)
        flb = eng.upload(np.full((lay["total"] + 1) // 2, GARBAGE, dtype=np.uint64))
        check(lib.fhe_ctx_inject_fault_bgv_mod_switch(eng._h, 5, RESULT, R + 1, 17, 30))
        check(lib.fhe_bgv_hmult_checked(eng._h, ks._h, p0.ptr, p1.ptr, c.d[0].ptr, c.d[1].ptr, c.d[2].ptr, c.d[3].ptr, c.dk.ptr, 1, ab._h, flb.ptr, None))
        flat = flb.download().view(np.uint32)[:lay["total"]]
        assert np.flatnonzero(flat).tolist() == [lay["rescale"] + ml["scale_delta"][0] + R + 1]
        # a refused hook: nothing launched, not even the tensor step
        flb = eng.upload(np.full((lay["total"] + 1) // 2, GARBAGE, dtype=np.uint64))
        check(lib.fhe_ctx_inject_fault_bgv_mod_switch(eng._h, 4, SUM, 0, 0, 30))
        assert lib.fhe_bgv_hmult_checked(eng._h, ks._h, p0.ptr, p1.ptr, c.d[0].ptr, c.d[1].ptr, c.d[2].ptr, c.d[3].ptr, c.dk.ptr, 1, ab._h, flb.ptr, None) == UNSUPPORTED
        assert (flb.download() == GARBAGE).all()
        # a mod-switch hook stays armed through a multiply that does not switch, and fires in the next one that does
        check(lib.fhe_ctx_inject_fault_bgv_mod_switch(eng._h, 4, RESULT, 0, 0, 30))
        assert _raised(run(False)[2]) == []
        assert _raised(run()[2]) == [("rescale", "scale_last", 0)]
        assert _raised(run()[2]) == []
    eng.check()


def test_scope_limits_are_error_statuses(F, eng, cases):
    from fhe_reliability_gpu_amd._lib import check, lib, vp
    c = cases("A")
    ks, ab, N, L, K, R = c.ks, c.ab, c.N, c.L, c.K, c.R
    o0, o1, o = eng.alloc(L * N), eng.alloc(L * N), eng.alloc(3 * R * N)
    fl = eng.alloc(ks.bgv_hmult_checked_layout(True)["total"])
    d, dk = c.d, c.dk

    def every_call(plan, abft, flags=None):
        flags = fl.ptr if flags is None else flags
        return [lib.fhe_bgv_keyswitch_apply_checked(eng._h, plan, o0.ptr, o1.ptr, d[0].ptr, dk.ptr, None, None, abft, flags, None),
                lib.fhe_bgv_relinearize_checked(eng._h, plan, o0.ptr, o1.ptr, d[0].ptr, d[1].ptr, d[2].ptr, dk.ptr, abft, flags, None),
                lib.fhe_bgv_rotate_checked(eng._h, plan, o0.ptr, o1.ptr, d[0].ptr, d[1].ptr, 5, dk.ptr, abft, flags, None),
                lib.fhe_bgv_mod_switch_checked(eng._h, plan, o.ptr, c.dc3.ptr, 2, abft, flags, None),
                lib.fhe_bgv_hmult_checked(eng._h, plan, o0.ptr, o1.ptr, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, dk.ptr, 1, abft, flags, None),
                lib.fhe_bgv_hmult_checked(eng._h, plan, o0.ptr, o1.ptr, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, dk.ptr, 0, abft, flags, None)]

    def reason():
        return lib.fhe_last_error().decode()

    # a plan without a plain modulus
    assert every_call(ks._h, ab._h) == [INVALID] * 6 and "no plain modulus" in reason()
    with plain_modulus(ks, 65537):
        assert every_call(ks._h, ab._h) == [0] * 6
        # a one-rank sharded plan
        g1, g2, bc = eng.alloc(L * N), eng.alloc(2 * K * N), eng.alloc(3 * N)
        sh = vp()
        check(lib.fhe_keyswitch_create_sharded(eng._h, c.t._h, L, K, c.dnum, 1, 0, g1.ptr, g2.ptr, bc.ptr, C.byref(sh)))
        try:
            check(lib.fhe_keyswitch_set_plain_modulus(sh, 65537))
            assert every_call(sh, ab._h) == [INVALID] * 6 and "sharded" in reason()
        finally:
            lib.fhe_keyswitch_destroy(sh)
        # a detector made for another table set; null flags, null detector
        ab2 = F.Abft(eng, eng.tables(c.logn, c.qs))
        assert every_call(ks._h, ab2._h) == [INVALID] * 6 and "another table set" in reason()
        assert every_call(ks._h, None) == [INVALID] * 6 and every_call(ks._h, ab._h, flags=vp()) == [INVALID] * 6
        # ntt_mode = 1
        eng.set_option("ntt_mode", 1)
        try:
            assert every_call(ks._h, ab._h) == [UNSUPPORTED] * 6 and "ntt_mode" in reason()
        finally:
            eng.set_option("ntt_mode", 0)
        # a transform-stage hook at a one-launch size: refused, nothing left armed
        clean_ks = lambda: _raised(ks.bgv_apply_checked(d[0], dk, ab)[2]) == []
        clean_ms = lambda: _raised(ks.bgv_mod_switch_checked(c.dc3, ab)[1]) == []
        for stage in (0, 2, 4, 6):
            check(lib.fhe_ctx_inject_fault_bgv_keyswitch(eng._h, stage, 0, 0 if stage != 2 else L, 5, 30))
            assert every_call(ks._h, ab._h)[0] == UNSUPPORTED and "two-launch" in reason()
            assert clean_ks()
        for stage in (0, 2):
            check(lib.fhe_ctx_inject_fault_bgv_mod_switch(eng._h, stage, 0, 0, 5, 30))
            assert every_call(ks._h, ab._h)[3] == UNSUPPORTED and "two-launch" in reason()
            assert clean_ms()
        # stages the setters do not have; bad points and bits
        assert lib.fhe_ctx_inject_fault_bgv_keyswitch(eng._h, 8, 0, 0, 0, 0) == INVALID
        assert lib.fhe_ctx_inject_fault_bgv_keyswitch(eng._h, 11, 0, 0, 0, 0) == INVALID
        assert lib.fhe_ctx_inject_fault_bgv_keyswitch(eng._h, 9, 4, 0, 0, 0) == INVALID
        assert lib.fhe_ctx_inject_fault_bgv_mod_switch(eng._h, 6, 0, 0, 0, 0) == INVALID
        assert lib.fhe_ctx_inject_fault_bgv_mod_switch(eng._h, 4, 0, 0, 0, 64) == INVALID
        assert clean_ks() and clean_ms()
        # an armed non-BGV hook is neither taken nor honoured by a BGV call ...
        check(lib.fhe_ctx_inject_fault_keyswitch(eng._h, 7, RESULT, 0, 3, 30))
        check(lib.fhe_ctx_inject_fault_rescale(eng._h, 1, RESULT, 0, 3, 30))
        assert clean_ks() and clean_ms()
        assert _raised(ks.bgv_hmult_checked(*d, dk, ab)[2]) == []
    # ... it still fires in the next non-BGV checked call on the plan without plain modulus
    assert _raised(ks.apply_checked(d[0], dk, ab)[2]) == [("", "tail", 0)]
    assert _raised(ks.rescale_checked(c.dc3, ab)[1]) == [("", "reduce", 0)]
    # and a BGV hook is not taken by the non-BGV calls
    check(lib.fhe_ctx_inject_fault_bgv_keyswitch(eng._h, 7, RESULT, 1, 3, 30))
    assert _raised(ks.apply_checked(d[0], dk, ab)[2]) == []
    with plain_modulus(ks, 65537):
        assert _raised(ks.bgv_apply_checked(d[0], dk, ab)[2]) == [("", "tail", 1)]
    eng.check()


def _affine_want(a, qs, mul, add):
    """Python integers: a = [n_poly][limbs][N]"""
    out = np.zeros_like(a)
    for l, q in enumerate(qs):
        s, o = (1 if mul is None else int(mul[l]) % q), (0 if add is None else int(add[l]) % q)
        out[:, l] = np.array([[(int(v) * s + o) % q for v in row] for row in a[:, l]], dtype=np.uint64)
    return out


def test_scalar_affine_checked_words_flags_and_hook(F, eng, cases):
    from fhe_reliability_gpu_amd._lib import check, lib
    c = cases("B")
    t, N = c.t, c.N
    start, limbs = 1, 2                              # the 61-bit limb and a 50-bit one
    qs = c.qs[start:start + limbs]
    rng = np.random.default_rng(7)
    p64 = C.POINTER(C.c_uint64)
    arr = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.uint64)
    ptr = lambda v: None if v is None else v.ctypes.data_as(p64)
    for n_poly in (1, 3):
        a = np.stack([np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs]) for _ in range(n_poly)])
        a[0, :, :3] = [[0, 1, q - 1] for q in qs]
        # scalars as a caller may hand them over: not reduced
        mul, add = [2**64 - 1, 65537], [q - 1 for q in qs]
        for m, o in ((mul, add), (None, add), (mul, None), (None, None)):
            da, dcc = eng.upload(a), eng.alloc(a.size)
            f = t.scalar_affine_checked(dcc, da, m, o, limbs=limbs, start=start, n_poly=n_poly)
            assert f.shape == (n_poly * limbs,) and not f.any()
            want = _affine_want(a, qs, m, o)
            assert (dcc.download().reshape(a.shape) == want).all() and (da.download() == a).all()
            f = t.scalar_affine_checked(da, da, m, o, limbs=limbs, start=start, n_poly=n_poly)      # in place
            assert not f.any() and (da.download() == want).all()
            un = eng.alloc(a.size)
            check(lib.fhe_scalar_affine(eng._h, un.ptr, eng.upload(a).ptr, ptr(arr(m)), ptr(arr(o)), t._h, n_poly, limbs, start, None))
            assert (un.download().reshape(a.shape) == want).all()
    # words that are not residues: bit 4 alone on their units, the words fhe_scalar_affine's
    a = np.stack([np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs]) for _ in range(3)])
    a[0, 1, 5], a[2, 0, N - 1], a[2, 0, 0] = 2**64 - 1, qs[0], qs[0] + 12345
    for m, o in (([3, 786433], [1, 2]), ([3, 786433], None)):
        da, dcc, un = eng.upload(a), eng.alloc(a.size), eng.alloc(a.size)
        f = t.scalar_affine_checked(dcc, da, m, o, limbs=limbs, start=start, n_poly=3)
        assert f.tolist() == [0, OPERAND, 0, 0, OPERAND, 0]
        check(lib.fhe_scalar_affine(eng._h, un.ptr, da.ptr, ptr(arr(m)), ptr(arr(o)), t._h, 3, limbs, start, None))
        assert (dcc.download() == un.download()).all()
    # 65 limbs: refused before anything is touched
    flb = eng.upload(np.full(40, GARBAGE, dtype=np.uint64))
    da = eng.upload(a)
    assert lib.fhe_scalar_affine_checked(eng._h, da.ptr, da.ptr, None, None, t._h, 1, 65, 0, flb.ptr, None) == UNSUPPORTED
    assert (flb.download() == GARBAGE).all() and (da.download() == a).all()
    # the pointwise hook: element (poly 1, limb 1, coefficient 9) -> unit 3
    a = np.stack([np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs]) for _ in range(2)])
    idx, unit = (1 * limbs + 1) * N + 9, 3
    for o in ([5, 6], None):
        want = _affine_want(a, qs, [3, 786433], o)
        for point, bit in ((PRODUCT, 30), (QUOTIENT, 21), (RESULT, 30), (SUM, 30)):
            da, dcc = eng.upload(a), eng.alloc(a.size)
            check(lib.fhe_ctx_inject_fault_pointwise(eng._h, point, idx, bit))
            if point == SUM and o is None:
                flb = eng.upload(np.full(2, GARBAGE, dtype=np.uint64))
                assert lib.fhe_scalar_affine_checked(eng._h, dcc.ptr, da.ptr, ptr(arr([3, 786433])), None, t._h, 2, limbs, start, flb.ptr, None) == UNSUPPORTED
                assert (flb.download() == GARBAGE).all()
            else:
                f = t.scalar_affine_checked(dcc, da, [3, 786433], o, limbs=limbs, start=start, n_poly=2)
                assert np.flatnonzero(f).tolist() == [unit], (point, f)
                got = dcc.download().reshape(a.shape)
                assert got[1, 1, 9] != want[1, 1, 9] and (np.flatnonzero(got != want).size == 1)
            f = t.scalar_affine_checked(dcc, da, [3, 786433], o, limbs=limbs, start=start, n_poly=2)      # used up either way
            assert not f.any() and (dcc.download().reshape(a.shape) == want).all()
    # an index outside the call
    check(lib.fhe_ctx_inject_fault_pointwise(eng._h, RESULT, 2 * limbs * N, 0))
    flb = eng.upload(np.full(2, GARBAGE, dtype=np.uint64))
    assert lib.fhe_scalar_affine_checked(eng._h, dcc.ptr, da.ptr, None, None, t._h, 2, limbs, start, flb.ptr, None) == INVALID
    eng.check()
