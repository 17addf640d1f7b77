"""Stage-by-stage checked rescale and the one-call checked homomorphic multiply on the GPU: clean calls return the unchecked
calls' words bit for bit (and the oracle's at the smaller sizes) with every flag zero from a garbage-filled buffer; one armed bit
flip at (stage, unit) raises exactly that flag word and no other -- in the rescale's layout and at the right offset of the
multiply's --, changes the outputs, and leaves the next call clean; the scope limits are error statuses."""
import ctypes as C

import numpy as np
import pytest

from helpers.checked_plan import checked_plan

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
PRODUCT, QUOTIENT, RESULT, SUM = 0, 1, 2, 3
KS_STAGES = ("intt_in", "extend", "ntt_ext", "mac", "intt_special", "moddown", "ntt_conv", "tail")
RS_STAGES = ("intt_last", "reduce", "ntt_delta", "scale")


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


def _setup(F, eng, logn, L, K, dnum, kind, seed):
    N = 1 << logn
    qs, t, ks, ab, rng = checked_plan(F, eng, logn, L, K, dnum, kind, seed)
    poly = lambda: np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs[:L]])
    ops = [poly() for _ in range(4)]
    rlk = np.stack([np.stack([np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs]) for _ in range(2)]) for _ in range(dnum)])
    return qs, t, ks, ab, ops, rlk


def _ks_total(L, K, dnum):
    M = L + K
    return L + 2 * dnum * M + 2 * M + 2 * K + 2 * (K + L) + 4 * L


def _all_words(flags):
    """[(block, stage, flat unit, value)] of every raised word of a rescale's or a multiply's flags"""
    out = []
    if "tensor" in flags:
        out += [("tensor", "tensor", int(u), int(flags["tensor"].reshape(-1)[u])) for u in np.flatnonzero(flags["tensor"].reshape(-1))]
        blocks = [("keyswitch", flags["keyswitch"])] + ([("rescale", flags["rescale"])] if flags["rescale"] is not None else [])
    else:
        blocks = [("rescale", flags)]
    for block, d in blocks:
        for name, f in d.items():
            out += [(block, name, int(u), int(f.reshape(-1)[u])) for u in np.flatnonzero(f.reshape(-1))]
    return out


def _clean_rescale(flags):
    assert sorted(flags) == sorted(RS_STAGES)
    assert _all_words(flags) == []


def _clean_hmult(flags, rescale):
    assert sorted(flags) == ["keyswitch", "rescale", "tensor"]
    assert sorted(flags["keyswitch"]) == sorted(KS_STAGES)
    assert (flags["rescale"] is None) == (not rescale)
    if rescale:
        assert sorted(flags["rescale"]) == sorted(RS_STAGES)
    assert _all_words(flags) == []


# drawn from CLEAN of test_gpu_keyswitch_checked.py: single-launch sizes from 2^5, two-launch sizes to 2^16, the kinds 50 / 61 / mixed,
# dnum = 1 / dnum = L / K = 1; the last plan has 3 (L - 1) = 21 > max(dnum, 2) (L + K) = 18 slots of ABFT sums
CLEAN = [(5, 3, 1, 3, "50"), (10, 4, 2, 2, "50"), (12, 6, 2, 3, "50"), (12, 4, 2, 4, "mixed"), (9, 5, 3, 2, "50/50"), (13, 3, 2, 1, "61/61"),
         (13, 4, 1, 4, "50/50"), (13, 5, 2, 3, "mixed"), (14, 3, 1, 3, "61"), (15, 4, 2, 2, "61"), (16, 3, 1, 3, "50"), (16, 4, 2, 2, "mixed"),
         (13, 8, 1, 1, "mixed")]


@pytest.mark.parametrize("logn,L,K,dnum,kind", CLEAN)
def test_clean_calls_return_the_unchecked_words_and_no_flag(F, eng, logn, L, K, dnum, kind):
    import torch
    from oracle.keyswitch_ref import hmult_ref, rescale_ref
    qs, t, ks, ab, (a0, a1, b0, b1), rlk = _setup(F, eng, logn, L, K, dnum, kind, logn * 89 + L * 5 + dnum)
    R = L - 1
    c3 = np.stack([a0, a1, b0])
    d = [eng.upload(v) for v in (a0, a1, b0, b1)]
    dk, dc = eng.upload(rlk), eng.upload(c3)
    # layouts against the closed forms
    for n_parts in (1, 2, 3):
        lay = ks.rescale_checked_layout(n_parts)
        assert lay["total"] == n_parts * (1 + 3 * R)
        assert [lay[s][0] for s in RS_STAGES] == [0, n_parts, n_parts * (1 + R), n_parts * (1 + 2 * R)]
    hl = ks.hmult_checked_layout(True)
    assert hl == {"tensor": 0, "keyswitch": 3 * L, "rescale": 3 * L + _ks_total(L, K, dnum), "total": 3 * L + _ks_total(L, K, dnum) + 2 * (1 + 3 * R)}
    hl0 = ks.hmult_checked_layout(False)
    assert hl0["total"] == hl0["rescale"] == 3 * L + _ks_total(L, K, dnum)
    assert ks.checked_layout()["total"] == _ks_total(L, K, dnum)
    user = torch.cuda.Stream()
    for stream in (None, C.c_void_p(user.cuda_stream)):
        for n_parts in (1, 2, 3):
            o, fl = ks.rescale_checked(dc, ab, n_parts=n_parts, stream=stream)
            _clean_rescale(fl)
            got = o.download()
            assert (got == ks.rescale(dc, n_parts=n_parts).download()).all(), f"n_parts {n_parts}"
            if stream is None and logn <= 12:
                assert (got.reshape(n_parts, R, -1) == rescale_ref(c3[:n_parts], qs, L, logn)).all()
        for rescale in (True, False):
            o0, o1, fl = ks.hmult_checked(*d, dk, ab, rescale=rescale, stream=stream)
            _clean_hmult(fl, rescale)
            g0, g1 = o0.download(), o1.download()
            for fused in (0, 1):
                eng.set_option("hmult_fused_rescale", fused)
                try:
                    u0, u1 = ks.hmult(*d, dk, rescale=rescale)
                    assert (g0 == u0.download()).all() and (g1 == u1.download()).all(), f"rescale {rescale} hmult_fused_rescale {fused}"
                finally:
                    eng.set_option("hmult_fused_rescale", 1)
            if stream is None and logn <= 12:
                w0, w1 = hmult_ref(a0, a1, b0, b1, rlk, qs, L, K, dnum, logn, rescale=rescale)
                assert (g0 == w0).all() and (g1 == w1).all()
        # inputs untouched
        assert all((x.download() == v).all() for x, v in zip(d, (a0, a1, b0, b1))) and (dc.download() == c3.reshape(dc.download().shape)).all()
        assert (dk.download() == rlk.reshape(dk.download().shape)).all()
    eng.check()


def _rescale_cases(L, n_parts, two_launch):
    """(stage, point, unit): every stage the size has, on the first and the last unit, on part 0 and the last part"""
    R = L - 1
    cases = [(1, PRODUCT, 0), (1, RESULT, n_parts * R - 1), (1, QUOTIENT, (n_parts - 1) * R), (1, RESULT, R - 1),
             (3, PRODUCT, 0), (3, RESULT, n_parts * R - 1), (3, QUOTIENT, (n_parts - 1) * R), (3, RESULT, R - 1)]
    if two_launch:
        cases += [(0, 0, 0), (0, 0, n_parts - 1), (2, 0, 0), (2, 0, n_parts * R - 1), (2, 0, (n_parts - 1) * R), (2, 0, R - 1)]
    return cases


@pytest.mark.parametrize("logn,kind", [(10, "mixed"), (13, "50/50"), (13, "61/61")])
def test_one_flip_in_the_rescale_raises_exactly_its_own_word(F, eng, logn, kind):
    from fhe_reliability_gpu_amd._lib import check, lib
    L, K, dnum = 4, 2, 2
    N, R = 1 << logn, L - 1
    qs, t, ks, ab, (a0, a1, b0, b1), rlk = _setup(F, eng, logn, L, K, dnum, kind, logn + len(kind))
    stages_hit = set()
    for n_parts in (3, 1):
        dc = eng.upload(np.stack([a0, a1, b0])[:n_parts])
        o, fl = ks.rescale_checked(dc, ab, n_parts=n_parts)
        _clean_rescale(fl)
        want = o.download()
        for i, (stage, point, unit) in enumerate(_rescale_cases(L, n_parts, logn >= 13)):
            # bit 30 of a product word, a stored word or a word between two launches always changes the result; bit 21 of the tail's
            # quotient estimate moves the remainder by 2^21 q; bit 44 of the residue stage's estimate (a quotient below 2^12 here)
            # leaves a word far outside [0, q) (the CPU emulation test covers every bit)
            bit = 44 if stage == 1 and point != RESULT else 21 if point == QUOTIENT else 30
            coeff = (0, N // 2 + 7, N - 1)[i % 3]
            check(lib.fhe_ctx_inject_fault_rescale(eng._h, stage, point, unit, coeff, bit))
            o, fl = ks.rescale_checked(dc, ab, n_parts=n_parts)
            hits = [(s, u) for _, s, u, _ in _all_words(fl)]
            assert hits == [(RS_STAGES[stage], unit)], f"n_parts {n_parts} stage {stage} point {point} unit {unit}: raised {_all_words(fl)}"
            assert (o.download() != want).any(), f"stage {stage} unit {unit}: outputs unchanged"
            o, fl = ks.rescale_checked(dc, ab, n_parts=n_parts)      # one shot: the next call is clean again
            _clean_rescale(fl)
            assert (o.download() == want).all()
            stages_hit.add(stage)
        if logn < 13:
            # the transform stages' hook needs a two-launch size: refused, nothing launched, nothing left armed
            o = eng.alloc(n_parts * R * N)
            flb = eng.alloc(ks.rescale_checked_layout(n_parts)["total"])
            for stage in (0, 2):
                check(lib.fhe_ctx_inject_fault_rescale(eng._h, stage, 0, 0, 5, 30))
                assert lib.fhe_rescale_checked(eng._h, ks._h, o.ptr, dc.ptr, n_parts, ab._h, flb.ptr, None) == UNSUPPORTED
                _clean_rescale(ks.rescale_checked(dc, ab, n_parts=n_parts)[1])
    assert stages_hit == ({0, 1, 2, 3} if logn >= 13 else {1, 3})
    eng.check()


def _hmult_expect(flags, block, stage, unit, what):
    hits = [(b, s, u) for b, s, u, _ in _all_words(flags)]
    assert hits == [(block, stage, unit)], f"{what}: raised {_all_words(flags)}"


@pytest.mark.parametrize("logn,kind", [(10, "mixed"), (13, "mixed")])
def test_one_flip_per_block_inside_hmult_checked(F, eng, logn, kind):
    """each of the three hooks fires in its own step, raises its own word at the right offset of the one buffer and nothing else"""
    from fhe_reliability_gpu_amd._lib import check, lib
    L, K, dnum = 4, 2, 2
    N, R, M = 1 << logn, L - 1, L + K
    qs, t, ks, ab, ops, rlk = _setup(F, eng, logn, L, K, dnum, kind, 3 * logn)
    d, dk = [eng.upload(v) for v in ops], eng.upload(rlk)
    o0, o1, fl = ks.hmult_checked(*d, dk, ab)
    _clean_hmult(fl, True)
    want = o0.download(), o1.download()

    def run(what, block, stage, unit, rescale=True):
        o0, o1, fl = ks.hmult_checked(*d, dk, ab, rescale=rescale)
        _hmult_expect(fl, block, stage, unit, what)
        if rescale:
            assert (o0.download() != want[0]).any() or (o1.download() != want[1]).any(), f"{what}: outputs unchanged"
            o0, o1, fl = ks.hmult_checked(*d, dk, ab)
            _clean_hmult(fl, True)
            assert (o0.download() == want[0]).all() and (o1.download() == want[1]).all()

    # tensor block: element (limb 2, coefficient 9) of d1 (its running sum) and of d0 / d2 (the result word)
    check(lib.fhe_ctx_inject_fault_pointwise(eng._h, SUM, 2 * N + 9, 30))
    run("tensor sum", "tensor", "tensor", 3 * 2 + 1)
    check(lib.fhe_ctx_inject_fault_pointwise(eng._h, SUM, 9, 30))
    run("tensor sum, no rescale", "tensor", "tensor", 1, rescale=False)
    # key-switch block: every residue-checked stage, and the transform stages at the two-launch size
    ks_cases = [(1, RESULT, 0), (3, PRODUCT, M + 1), (5, RESULT, 2 * (K + L) - 1), (7, SUM, L + 1)]
    if logn >= 13:
        ks_cases += [(0, 0, L - 1), (2, 0, M + 0), (4, 0, K), (6, 0, 2 * L - 1)]
    for stage, point, unit in ks_cases:
        check(lib.fhe_ctx_inject_fault_keyswitch(eng._h, stage, point, unit, N // 2 + 7, 30))
        run(f"key switch stage {stage}", "keyswitch", KS_STAGES[stage], unit)
    check(lib.fhe_ctx_inject_fault_keyswitch(eng._h, 7, RESULT, 0, 3, 30))
    run("key switch tail, no rescale", "keyswitch", "tail", 0, rescale=False)
    # rescale block (two parts): all four stages where the size has them
    rs_cases = [(1, RESULT, 0), (1, PRODUCT, 2 * R - 1), (3, PRODUCT, R), (3, RESULT, 2 * R - 1)]
    if logn >= 13:
        rs_cases += [(0, 0, 1), (2, 0, R + 1)]
    for stage, point, unit in rs_cases:
        bit = 44 if stage == 1 and point == PRODUCT else 30
        check(lib.fhe_ctx_inject_fault_rescale(eng._h, stage, point, unit, N - 1, bit))
        run(f"rescale stage {stage}", "rescale", RS_STAGES[stage], unit)
    # the offsets in the one buffer are the layout's: a raw call, flags read back flat
    lay = ks.hmult_checked_layout(True)
    rl = ks.rescale_checked_layout(2)
    o0, o1 = eng.alloc(R * N), eng.alloc(R * N)
    flb = eng.upload(np.full((lay["total"] + 1) // 2, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64))
    check(lib.fhe_ctx_inject_fault_rescale(eng._h, 3, RESULT, R + 2, 17, 30))
    check(lib.fhe_hmult_checked(eng._h, ks._h, o0.ptr, o1.ptr, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, dk.ptr, 1, ab._h, flb.ptr, None))
    flat = flb.download().view(np.uint32)[:lay["total"]]
    assert np.flatnonzero(flat).tolist() == [lay["rescale"] + rl["scale"][0] + R + 2]
    # a rescale hook stays armed through a multiply that does not rescale, and fires in the next rescale
    check(lib.fhe_ctx_inject_fault_rescale(eng._h, 1, RESULT, 0, 0, 30))
    _clean_hmult(ks.hmult_checked(*d, dk, ab, rescale=False)[2], False)
    _hmult_expect(ks.hmult_checked(*d, dk, ab)[2], "rescale", "reduce", 0, "armed through a multiply without rescale")
    _clean_hmult(ks.hmult_checked(*d, dk, ab)[2], True)
    eng.check()


def test_a_refused_rescale_hook_stops_the_multiply_before_its_first_launch(F, eng):
    """every hook is checked against the call before anything is enqueued: a rescale hook the call refuses leaves the flag buffer
    and both outputs as they were, and the next call is clean"""
    from fhe_reliability_gpu_amd._lib import check, lib
    logn, L, K, dnum = 10, 4, 2, 2
    N, R = 1 << logn, L - 1
    qs, t, ks, ab, ops, rlk = _setup(F, eng, logn, L, K, dnum, "mixed", 41)
    d, dk = [eng.upload(v) for v in ops], eng.upload(rlk)
    o0, o1, fl = ks.hmult_checked(*d, dk, ab)
    _clean_hmult(fl, True)
    want = o0.download(), o1.download()
    pattern = 0x5A5A5A5A5A5A5A5A
    total = ks.hmult_checked_layout(True)["total"]
    flb, p0, p1 = (eng.upload(np.full(n, pattern, dtype=np.uint64)) for n in ((total + 1) // 2, R * N, R * N))
    check(lib.fhe_ctx_inject_fault_rescale(eng._h, 1, SUM, 0, 0, 30))      # x mod q_j has no running sum
    assert lib.fhe_hmult_checked(eng._h, ks._h, p0.ptr, p1.ptr, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, dk.ptr, 1, ab._h, flb.ptr, None) == UNSUPPORTED
    eng.sync()
    assert all((x.download() == pattern).all() for x in (flb, p0, p1))
    o0, o1, fl = ks.hmult_checked(*d, dk, ab)
    _clean_hmult(fl, True)
    assert (o0.download() == want[0]).all() and (o1.download() == want[1]).all()
    eng.check()


def test_scope_limits_are_error_statuses(F, eng):
    from fhe_reliability_gpu_amd._lib import check, lib, vp
    logn, L, K, dnum = 10, 4, 2, 2
    N, R = 1 << logn, L - 1
    qs, t, ks, ab, (a0, a1, b0, b1), rlk = _setup(F, eng, logn, L, K, dnum, "50", 3)
    d = [eng.upload(v) for v in (a0, a1, b0, b1)]
    dk, dc = eng.upload(rlk), eng.upload(np.stack([a0, a1, b0]))
    o = eng.alloc(3 * R * N)
    o0, o1 = eng.alloc(L * N), eng.alloc(L * N)
    fl = eng.alloc(ks.hmult_checked_layout(True)["total"])

    def rescale(plan, abft, flags, out=None, n_parts=2):
        return lib.fhe_rescale_checked(eng._h, plan, (o if out is None else out).ptr, dc.ptr, n_parts, abft, flags, None)

    def hmult(plan, abft, flags, out0=None, out1=None, resc=1):
        p0, p1 = (o0 if out0 is None else out0).ptr, (o1 if out1 is None else out1).ptr
        return lib.fhe_hmult_checked(eng._h, plan, p0, p1, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, dk.ptr, resc, abft, flags, None)

    def reason():
        return lib.fhe_last_error().decode()

    assert rescale(ks._h, ab._h, fl.ptr) == 0 and hmult(ks._h, ab._h, fl.ptr) == 0
    # a sharded plan
    g1, g2, bc = eng.alloc(L * N), eng.alloc(2 * K * N), eng.alloc(3 * N)
    sh = vp()
    check(lib.fhe_keyswitch_create_sharded(eng._h, t._h, L, K, dnum, 1, 0, g1.ptr, g2.ptr, bc.ptr, C.byref(sh)))
    try:
        assert rescale(sh, ab._h, fl.ptr) == INVALID and "sharded" in reason()
        assert hmult(sh, ab._h, fl.ptr) == INVALID and "sharded" in reason()
    finally:
        lib.fhe_keyswitch_destroy(sh)
    # a plan with a plain modulus (BGV)
    ks.set_plain_modulus(65537)
    try:
        assert rescale(ks._h, ab._h, fl.ptr) == UNSUPPORTED and "plain modulus" in reason()
        assert hmult(ks._h, ab._h, fl.ptr) == UNSUPPORTED and "plain modulus" in reason()
    finally:
        ks.set_plain_modulus(0)
    # ntt_mode = 1
    eng.set_option("ntt_mode", 1)
    try:
        assert rescale(ks._h, ab._h, fl.ptr) == UNSUPPORTED and "ntt_mode" in reason()
        assert hmult(ks._h, ab._h, fl.ptr) == UNSUPPORTED and "ntt_mode" in reason()
    finally:
        eng.set_option("ntt_mode", 0)
    # L = 1: no prime left to drop (a multiply that does not rescale is fine)
    t1 = eng.tables(logn, qs[:1] + qs[L:])
    ks1, ab1 = F.KeySwitch(eng, t1, 1, K, 1), F.Abft(eng, t1)
    rlk1 = eng.upload(np.zeros((1, 2, 1 + K, N), dtype=np.uint64))
    lay = (C.c_int * 6)()
    assert lib.fhe_rescale_checked_layout(ks1._h, 2, lay) == INVALID
    assert lib.fhe_hmult_checked_layout(ks1._h, 1, lay) == INVALID
    assert rescale(ks1._h, ab1._h, fl.ptr) == INVALID and "no prime left" in reason()
    call1 = lambda resc: lib.fhe_hmult_checked(eng._h, ks1._h, o0.ptr, o1.ptr, d[0].ptr, d[0].ptr, d[0].ptr, d[0].ptr, rlk1.ptr, resc, ab1._h, fl.ptr, None)
    assert call1(1) == INVALID and "no prime left" in reason()
    assert call1(0) == 0
    # a detector made for another table set
    ab2 = F.Abft(eng, eng.tables(logn, qs))
    assert rescale(ks._h, ab2._h, fl.ptr) == INVALID and "another table set" in reason()
    assert hmult(ks._h, ab2._h, fl.ptr) == INVALID and "another table set" in reason()
    # null flags, null detector
    assert rescale(ks._h, ab._h, None) == INVALID and rescale(ks._h, None, fl.ptr) == INVALID
    assert hmult(ks._h, ab._h, None) == INVALID and hmult(ks._h, None, fl.ptr) == INVALID
    # the two outputs of a multiply must be distinct
    assert hmult(ks._h, ab._h, fl.ptr, out0=o0, out1=o0) == INVALID and "distinct" in reason()
    # an output of the rescale that overlaps its input; part counts
    assert rescale(ks._h, ab._h, fl.ptr, out=dc) == INVALID and "out of place" in reason()
    for n_parts in (0, 4):
        assert rescale(ks._h, ab._h, fl.ptr, n_parts=n_parts) == INVALID and "1 to 3 parts" in reason()
        assert lib.fhe_rescale_checked_layout(ks._h, n_parts, lay) == INVALID
    # bad hooks: a stage or point that does not exist; a unit or coefficient outside the call; the points the stages do not have
    assert lib.fhe_ctx_inject_fault_rescale(eng._h, 4, 0, 0, 0, 0) == INVALID
    assert lib.fhe_ctx_inject_fault_rescale(eng._h, 1, 4, 0, 0, 0) == INVALID
    assert lib.fhe_ctx_inject_fault_rescale(eng._h, 1, 0, 0, 0, 64) == INVALID
    for stage, point, unit, coeff, status in ((1, RESULT, 2 * R, 0, INVALID), (3, RESULT, 2 * R, 0, INVALID), (1, RESULT, 0, N, INVALID),
                                              (0, 0, 2, 0, INVALID), (1, SUM, 0, 0, UNSUPPORTED), (3, SUM, 0, 0, UNSUPPORTED)):
        check(lib.fhe_ctx_inject_fault_rescale(eng._h, stage, point, unit, coeff, 30))
        assert rescale(ks._h, ab._h, fl.ptr) == status, (stage, point, unit, coeff)
        _clean_rescale(ks.rescale_checked(dc, ab)[1])                 # used up by the refused call
        check(lib.fhe_ctx_inject_fault_rescale(eng._h, stage, point, unit, coeff, 30))
        assert hmult(ks._h, ab._h, fl.ptr) == status, (stage, point, unit, coeff)
        _clean_hmult(ks.hmult_checked(*d, dk, ab)[2], True)
    # a unit inside a three-part rescale is outside a two-part one
    check(lib.fhe_ctx_inject_fault_rescale(eng._h, 1, RESULT, 2 * R, 0, 30))
    assert rescale(ks._h, ab._h, fl.ptr, n_parts=3) == 0
    # clearing an armed hook
    check(lib.fhe_ctx_inject_fault_rescale(eng._h, 1, RESULT, 0, 0, 30))
    check(lib.fhe_ctx_inject_fault_rescale(eng._h, -1, 0, 0, 0, 0))
    _clean_rescale(ks.rescale_checked(dc, ab)[1])
    eng.check()


def test_config4_hmult_checked_matches_fhe_hmult_and_localises_a_fault():
    """N = 2^17, L = 32, K = 8, dnum = 4 (BASELINE config 4): multiply -> relinearize -> mod_switch_to_next as one checked call."""
    import fhe_reliability_gpu_amd as F
    from fhe_reliability_gpu_amd._lib import check, lib
    eng = F.default_engine()
    logn, L, K, dnum = 17, 32, 8, 4
    N, R = 1 << logn, L - 1
    qs = F.create_moduli(N, [50] * L + [61] * K)
    t = eng.tables(logn, qs)
    ks, ab = F.KeySwitch(eng, t, L, K, dnum), F.Abft(eng, t)
    rng = np.random.default_rng(4)
    lim = min(qs)
    up = lambda *shape: eng.upload(rng.integers(0, lim, shape, dtype=np.uint64))
    d = [up(L, N) for _ in range(4)]
    rk = up(dnum, 2, L + K, N)
    o0, o1, fl = ks.hmult_checked(*d, rk, ab)
    _clean_hmult(fl, True)
    u0, u1 = ks.hmult(*d, rk)
    want = u0.download(), u1.download()
    assert (o0.download() == want[0]).all() and (o1.download() == want[1]).all()
    unit = R + 17                                   # part 1, limb 17
    check(lib.fhe_ctx_inject_fault_rescale(eng._h, 1, RESULT, unit, N - 3, 30))
    o0, o1, fl = ks.hmult_checked(*d, rk, ab)
    _hmult_expect(fl, "rescale", "reduce", unit, "config 4, stage 1")
    assert (o0.download() == want[0]).all() and (o1.download()[17] != want[1][17]).any()
    o0, o1, fl = ks.hmult_checked(*d, rk, ab)
    _clean_hmult(fl, True)
    assert (o0.download() == want[0]).all() and (o1.download() == want[1]).all()
    eng.check()
