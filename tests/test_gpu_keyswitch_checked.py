"""Stage-by-stage checked key switch, relinearisation and rotation on the GPU: clean calls return the unchecked calls' words bit
for bit (and the oracle composite's) with every flag zero from a garbage-filled buffer; one armed bit flip at (stage, unit)
raises exactly that flag word and no other, changes the outputs, and leaves the next call clean; the scope limits are error
statuses."""
import ctypes as C

import numpy as np
import pytest

from helpers.checked_plan import checked_plan

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
PRODUCT, QUOTIENT, RESULT, SUM = 0, 1, 2, 3
STAGES = ("intt_in", "extend", "ntt_ext", "mac", "intt_special", "moddown", "ntt_conv", "tail")


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
    c0, c1, c2 = poly(), poly(), poly()
    evk = np.stack([np.stack([np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs]) for _ in range(2)]) for _ in range(dnum)])
    return qs, t, ks, ab, (c0, c1, c2), evk


def _clean(flags):
    assert sorted(flags) == sorted(STAGES)
    for name, f in flags.items():
        assert not f.any(), f"stage {name}: flags {np.argwhere(f != 0).tolist()} = {f[f != 0].tolist()} on a clean run"


def _same(a, b):
    return (a[0].download() == b[0].download()).all() and (a[1].download() == b[1].download()).all()


# the shapes of test_keyswitch_matches_oracle_composite first; one-limb digits (dnum = L) and K = 1; dnum > 8 with two-limb digits; all
# 50-bit, all 61-bit and mixed limbs with special primes of the other path; N from 2^5 (single launch) to 2^16 (two launches)
CLEAN = [(10, 4, 1, 4, "50"), (10, 4, 2, 2, "50"), (12, 6, 2, 3, "50"), (13, 3, 2, 1, "61/61"),
         (13, 4, 1, 4, "50/50"), (14, 3, 1, 3, "61"), (10, 22, 2, 11, "50"), (10, 22, 2, 11, "mixed"), (11, 9, 3, 9, "61"),
         (5, 3, 1, 3, "50"), (6, 4, 2, 2, "mixed"), (8, 3, 2, 2, "61"), (9, 5, 3, 2, "50/50"), (12, 4, 2, 4, "mixed"), (13, 5, 2, 3, "mixed"),
         (14, 5, 2, 3, "50"), (15, 4, 2, 2, "61"), (16, 3, 1, 3, "50"), (16, 4, 2, 2, "mixed"),
         # one digit: stages 4 and 6 address [2][M] and [2][L] sums, more than the dnum x M of stage 2
         (13, 6, 3, 1, "mixed"), (16, 24, 8, 1, "50")]


@pytest.mark.parametrize("logn,L,K,dnum,kind", CLEAN)
def test_clean_calls_return_the_unchecked_words_and_no_flag(F, eng, logn, L, K, dnum, kind):
    import torch
    from oracle.keyswitch_ref import keyswitch_ref
    qs, t, ks, ab, (c0, c1, c2), evk = _setup(F, eng, logn, L, K, dnum, kind, logn * 97 + L * 7 + dnum)
    N = 1 << logn
    d0, d1, d2, dk = eng.upload(c0), eng.upload(c1), eng.upload(c2), eng.upload(evk)
    lay = ks.checked_layout()
    M = L + K
    assert lay["total"] == L + 2 * dnum * M + 2 * M + 2 * K + 2 * (K + L) + 4 * L
    assert [lay[s][0] for s in STAGES] == list(np.cumsum([0, L, dnum * M, dnum * M, 2 * M, 2 * K, 2 * (K + L), 2 * L]))
    user = torch.cuda.Stream()
    for stream in (None, C.c_void_p(user.cuda_stream)):
        # key switch
        o = ks.apply_checked(d2, dk, ab, stream=stream)
        _clean(o[2])
        assert _same(o, ks.apply(d2, dk))
        if stream is None and logn <= 13:
            w0, w1 = keyswitch_ref(c2, evk, qs, L, K, dnum, logn)
            assert (o[0].download() == w0).all() and (o[1].download() == w1).all()
        # one addend only
        o = ks.apply_checked(d2, dk, ab, add0=d0, stream=stream)
        _clean(o[2])
        if stream is None and logn <= 12:
            w0, w1 = keyswitch_ref(c2, evk, qs, L, K, dnum, logn, add0=c0)
            assert (o[0].download() == w0).all() and (o[1].download() == w1).all()
        # relinearisation
        o = ks.relinearize_checked(d0, d1, d2, dk, ab, stream=stream)
        _clean(o[2])
        assert _same(o, ks.relinearize(d0, d1, d2, dk))
        # rotation
        for g in (3, 2 * N - 1):
            o = ks.rotate_checked(d0, d1, g, dk, ab, stream=stream)
            _clean(o[2])
            assert _same(o, ks.rotate(d0, d1, g, dk)), f"galois element {g}"
        assert (d0.download() == c0).all() and (d1.download() == c1).all() and (d2.download() == c2).all()      # inputs untouched
    eng.check()


def _big(F, eng, logn, L, K, dnum, seed):
    N = 1 << logn
    qs = F.create_moduli(N, [50] * L + [61] * K)
    t = eng.tables(logn, qs)
    rng = np.random.default_rng(seed)
    lim = min(qs)
    up = lambda *shape: eng.upload(rng.integers(0, lim, shape, dtype=np.uint64))
    return t, F.KeySwitch(eng, t, L, K, dnum), F.Abft(eng, t), up


def test_config5_rotation_matches_fhe_rotate():
    """N = 2^16, L = 44, K = 11, dnum = 4 (BASELINE config 5): the checked rotation against fhe_rotate on a sample of limbs."""
    import fhe_reliability_gpu_amd as F
    eng = F.default_engine()
    logn, L, K, dnum = 16, 44, 11, 4
    t, ks, ab, up = _big(F, eng, logn, L, K, dnum, 5)
    c0, c1, gk = up(L, 1 << logn), up(L, 1 << logn), up(dnum, 2, L + K, 1 << logn)
    o = ks.rotate_checked(c0, c1, 5, gk, ab)
    _clean(o[2])
    r = ks.rotate(c0, c1, 5, gk)
    for part in range(2):
        got, want = o[part].download(), r[part].download()
        for limb in (0, 1, 10, 11, 21, 33, 43):
            assert (got[limb] == want[limb]).all(), (part, limb)
    eng.check()


def test_config4_relinearisation_matches_fhe_relinearize():
    """N = 2^17, L = 32, K = 8, dnum = 4 (BASELINE config 4)."""
    import fhe_reliability_gpu_amd as F
    eng = F.default_engine()
    logn, L, K, dnum = 17, 32, 8, 4
    t, ks, ab, up = _big(F, eng, logn, L, K, dnum, 4)
    d0, d1, d2, rk = up(L, 1 << logn), up(L, 1 << logn), up(L, 1 << logn), up(dnum, 2, L + K, 1 << logn)
    o = ks.relinearize_checked(d0, d1, d2, rk, ab)
    _clean(o[2])
    assert _same(o, ks.relinearize(d0, d1, d2, rk))
    eng.check()


def _units(stage, L, K, dnum):
    """a first, a middle and a last unit of the stage's flags (flat index), covering both halves where the stage has halves"""
    M, alpha = L + K, (L + dnum - 1) // dnum
    if stage == 0:
        return [0, L // 2, L - 1]
    if stage == 1:                  # (0, 0): digit unit 0; (1, alpha + 1): digit unit 1 of digit 1; last: an output unit
        return [0, M + alpha + 1, dnum * M - 1]
    if stage == 2:                  # never one of the digit's own limbs
        return [alpha, M + 0, dnum * M - 1]
    if stage == 3:
        return [0, M + 1, 2 * M - 1]
    if stage == 4:
        return [0, K, 2 * K - 1]
    if stage == 5:                  # half 0 digit unit 0, half 1 digit unit 1, half 1 last output unit
        return [0, (K + L) + 1, 2 * (K + L) - 1]
    return [0, L + 1, 2 * L - 1]


@pytest.mark.parametrize("kind", ["50/50", "61/61"])
@pytest.mark.parametrize("logn", [13, 14])
def test_one_flip_raises_exactly_its_own_stage_and_unit(F, eng, logn, kind):
    from fhe_reliability_gpu_amd._lib import check, lib
    L, K, dnum = 4, 2, 2
    N = 1 << logn
    qs, t, ks, ab, (c0, c1, c2), evk = _setup(F, eng, logn, L, K, dnum, kind, logn + len(kind))
    d0, d1, d2, dk = eng.upload(c0), eng.upload(c1), eng.upload(c2), eng.upload(evk)
    clean = ks.relinearize_checked(d0, d1, d2, dk, ab)
    _clean(clean[2])
    want = clean[0].download(), clean[1].download()
    lay = ks.checked_layout()
    # (bit 30 of a product word, a running sum or a stored word always changes the word and leaves it canonical for the next stage;
    # a quotient flip may be absorbed by the conditional subtraction, which the CPU emulation test covers bit by bit)
    points = {1: [RESULT, PRODUCT, SUM], 5: [RESULT, SUM, PRODUCT], 3: [PRODUCT, SUM, RESULT], 7: [SUM, RESULT, PRODUCT]}
    n_cases = 0
    for stage in range(8):
        for i, unit in enumerate(_units(stage, L, K, dnum)):
            point = points[stage][i] if stage in points else 0
            bit, coeff = 30, (0, N // 2 + 7, N - 1)[i]
            check(lib.fhe_ctx_inject_fault_keyswitch(eng._h, stage, point, unit, coeff, bit))
            o0, o1, flags = ks.relinearize_checked(d0, d1, d2, dk, ab)
            for s, name in enumerate(STAGES):
                f = flags[name].reshape(-1)
                hit = np.flatnonzero(f)
                if s == stage:
                    assert hit.tolist() == [unit], f"stage {stage} unit {unit} point {point}: its own stage raised {hit.tolist()}"
                else:
                    assert hit.size == 0, f"stage {stage} unit {unit} point {point}: stage {s} raised {hit.tolist()}"
            assert (o0.download() != want[0]).any() or (o1.download() != want[1]).any(), f"stage {stage} unit {unit}: outputs unchanged"
            # one shot: the next call is clean again
            o0, o1, flags = ks.relinearize_checked(d0, d1, d2, dk, ab)
            _clean(flags)
            assert (o0.download() == want[0]).all() and (o1.download() == want[1]).all()
            n_cases += 1
    assert n_cases == 24
    eng.check()


def _expect_exactly(flags, stage, unit, what):
    for s, name in enumerate(STAGES):
        hit = np.flatnonzero(flags[name].reshape(-1))
        if s == stage:
            assert hit.tolist() == [unit], f"{what}: its own stage raised {hit.tolist()}"
        else:
            assert hit.size == 0, f"{what}: stage {s} raised {hit.tolist()}"


# (shape, call, cases (stage, point, unit as (index tuple into the stage's flags)))
# one-limb conversions (dnum = L, K = 1): the m = 1 checked conversion has points 0-2, and they raise their unit;
# key switch without addends: the tail's hook on a half without addend; dnum = 11: a fold of the running sum (after the eighth term)
# lies between a flip of the first term's product and the check
def _more_cases(L, K, dnum):
    M = L + K
    if dnum == L:
        return [(1, RESULT, 0), (1, PRODUCT, M + 0), (1, RESULT, dnum * M - 1), (1, QUOTIENT, 2 * M + 2),
                (5, PRODUCT, 0), (5, RESULT, (K + L) + K + 1), (5, PRODUCT, 2 * (K + L) - 1),
                (3, PRODUCT, 1), (3, SUM, M + L), (7, PRODUCT, 0), (7, RESULT, 2 * L - 1)]
    return [(3, PRODUCT, 0), (3, PRODUCT, M + L + 1), (3, SUM, M - 1), (3, RESULT, 2 * M - 1), (3, PRODUCT, M + 9),
            (7, SUM, 3), (7, PRODUCT, L + 2), (7, RESULT, 2 * L - 1), (2, 0, 5 * M + 1), (1, SUM, 10 * M + 21)]


@pytest.mark.parametrize("kind", ["50/50", "61/61"])
@pytest.mark.parametrize("L,K,dnum", [(4, 1, 4), (22, 2, 11)])
def test_flips_on_one_limb_conversions_without_addend_and_across_a_fold(F, eng, L, K, dnum, kind):
    from fhe_reliability_gpu_amd._lib import check, lib
    logn = 13
    N = 1 << logn
    qs, t, ks, ab, (c0, c1, c2), evk = _setup(F, eng, logn, L, K, dnum, kind, L + len(kind))
    d0, d2, dk = eng.upload(c0), eng.upload(c2), eng.upload(evk)
    # one-limb shape: no addend at all; dnum = 11: an addend on half 0 only
    call = (lambda: ks.apply_checked(d2, dk, ab)) if dnum == L else (lambda: ks.apply_checked(d2, dk, ab, add0=d0))
    clean = call()
    _clean(clean[2])
    want = clean[0].download(), clean[1].download()
    for i, (stage, point, unit) in enumerate(_more_cases(L, K, dnum)):
        # a quotient flip of a one-term Shoup product: bit 0 can be absorbed, bit 21 moves the remainder by 2^21 q (mod 2^64)
        bit, coeff = (30, 21, 12)[i % 3] if stage & 1 and point != QUOTIENT else (21 if point == QUOTIENT else 30), (i * 977 + 5) % N
        check(lib.fhe_ctx_inject_fault_keyswitch(eng._h, stage, point, unit, coeff, bit))
        o0, o1, flags = call()
        _expect_exactly(flags, stage, unit, f"stage {stage} point {point} unit {unit} bit {bit}")
        assert (o0.download() != want[0]).any() or (o1.download() != want[1]).any(), f"stage {stage} unit {unit}: outputs unchanged"
        o0, o1, flags = call()
        _clean(flags)
        assert (o0.download() == want[0]).all() and (o1.download() == want[1]).all()
    # points that do not exist here: the running sum of a one-term conversion, the tail's running sum on a half without addend
    o0, o1 = eng.alloc(L * N), eng.alloc(L * N)
    fl = eng.alloc(ks.checked_layout()["total"])
    refused = [(7, SUM, L)] + ([(1, SUM, 0), (1, SUM, 1), (5, SUM, 0), (5, SUM, 2), (7, SUM, 0)] if dnum == L else [(1, SUM, 0)])
    for stage, point, unit in refused:
        check(lib.fhe_ctx_inject_fault_keyswitch(eng._h, stage, point, unit, 0, 30))
        rc = lib.fhe_keyswitch_apply_checked(eng._h, ks._h, o0.ptr, o1.ptr, d2.ptr, dk.ptr, d0.ptr if dnum != L else None, None, ab._h, fl.ptr, None)
        assert rc == UNSUPPORTED, (stage, point, unit)
    _clean(call()[2])
    eng.check()


def test_scope_limits_are_error_statuses(F, eng):
    from fhe_reliability_gpu_amd._lib import check, lib, vp
    logn, L, K, dnum = 10, 4, 2, 2
    N = 1 << logn
    qs, t, ks, ab, (c0, c1, c2), evk = _setup(F, eng, logn, L, K, dnum, "50", 3)
    d0, d1, d2, dk = eng.upload(c0), eng.upload(c1), eng.upload(c2), eng.upload(evk)
    o0, o1 = eng.alloc(L * N), eng.alloc(L * N)
    fl = eng.alloc(ks.checked_layout()["total"])

    def apply(plan, abft, flags):
        return lib.fhe_keyswitch_apply_checked(eng._h, plan, o0.ptr, o1.ptr, d2.ptr, dk.ptr, None, None, abft, flags, None)

    assert apply(ks._h, ab._h, fl.ptr) == 0
    # a sharded plan (one rank with gather buffers runs the phase path)
    g1, g2 = eng.alloc(L * N), eng.alloc(2 * K * N)
    sh = vp()
    check(lib.fhe_keyswitch_create_sharded(eng._h, t._h, L, K, dnum, 1, 0, g1.ptr, g2.ptr, None, C.byref(sh)))
    try:
        assert apply(sh, ab._h, fl.ptr) == INVALID
        assert lib.fhe_rotate_checked(eng._h, sh, o0.ptr, o1.ptr, d0.ptr, d1.ptr, 3, dk.ptr, ab._h, fl.ptr, None) == INVALID
        lay = (C.c_int * 10)()
        assert lib.fhe_keyswitch_checked_layout(sh, lay) == 0
    finally:
        lib.fhe_keyswitch_destroy(sh)
    # a plan with a plain modulus
    ks.set_plain_modulus(65537)
    try:
        assert apply(ks._h, ab._h, fl.ptr) == UNSUPPORTED
        assert lib.fhe_relinearize_checked(eng._h, ks._h, o0.ptr, o1.ptr, d0.ptr, d1.ptr, d2.ptr, dk.ptr, ab._h, fl.ptr, None) == UNSUPPORTED
    finally:
        ks.set_plain_modulus(0)
    # a detector of another table set
    t2 = eng.tables(logn, qs)
    ab2 = F.Abft(eng, t2)
    assert apply(ks._h, ab2._h, fl.ptr) == INVALID
    # null flags, null detector
    assert apply(ks._h, ab._h, None) == INVALID
    assert apply(ks._h, None, fl.ptr) == INVALID
    # the transform stages' hook needs a two-launch size: refused, nothing launched, nothing left armed
    for stage in (0, 2, 4, 6):
        check(lib.fhe_ctx_inject_fault_keyswitch(eng._h, stage, 0, 0 if stage != 2 else L // dnum, 5, 30))
        assert apply(ks._h, ab._h, fl.ptr) == UNSUPPORTED
        o = ks.apply_checked(d2, dk, ab)
        _clean(o[2])
    # an armed hook is used up by a refused call too
    check(lib.fhe_ctx_inject_fault_keyswitch(eng._h, 3, RESULT, 0, 0, 30))
    assert apply(ks._h, ab._h, None) == INVALID
    o = ks.apply_checked(d2, dk, ab)
    _clean(o[2])
    assert _same(o, ks.apply(d2, dk))
    # bad hooks: a stage that does not exist, a unit outside the call, the tail's running sum on a half without addend
    assert lib.fhe_ctx_inject_fault_keyswitch(eng._h, 8, 0, 0, 0, 0) == INVALID
    assert lib.fhe_ctx_inject_fault_keyswitch(eng._h, 3, 4, 0, 0, 0) == INVALID
    check(lib.fhe_ctx_inject_fault_keyswitch(eng._h, 3, RESULT, 2 * (L + K), 0, 30))
    assert apply(ks._h, ab._h, fl.ptr) == INVALID
    check(lib.fhe_ctx_inject_fault_keyswitch(eng._h, 7, SUM, 0, 0, 30))
    assert apply(ks._h, ab._h, fl.ptr) == UNSUPPORTED
    o = ks.apply_checked(d2, dk, ab)
    _clean(o[2])
    # the context's transform variants the checked call does not run
    eng.set_option("ntt_resident", 1)
    try:
        assert apply(ks._h, ab._h, fl.ptr) == UNSUPPORTED
    finally:
        eng.set_option("ntt_resident", 0)
    eng.check()


def test_noncanonical_caller_words_raise_bit_4_alone(F, eng):
    """Only caller-supplied words can be out of range: a key word and an addend >= q raise bit 4 on their unit, nothing else, and the
    outputs are still the unchecked call's."""
    logn, L, K, dnum = 13, 4, 2, 2
    N = 1 << logn
    qs, t, ks, ab, (c0, c1, c2), evk = _setup(F, eng, logn, L, K, dnum, "mixed", 11)
    evk = evk.copy()
    evk[1, 1, 4, 99] = qs[4] + 5                     # key: digit 1, half 1, row 4 (a special limb)
    c0 = c0.copy()
    c0[2, 7] = np.uint64(2**64 - 1)                  # addend of half 0, limb 2
    d0, d1, d2, dk = eng.upload(c0), eng.upload(c1), eng.upload(c2), eng.upload(evk)
    o = ks.relinearize_checked(d0, d1, d2, dk, ab)
    assert _same(o, ks.relinearize(d0, d1, d2, dk))
    M = L + K
    for name, f in o[2].items():
        f = f.reshape(-1)
        if name == "mac":
            assert np.flatnonzero(f).tolist() == [M + 4] and f[M + 4] == 4
        elif name == "tail":
            assert np.flatnonzero(f).tolist() == [2] and f[2] == 4
        else:
            assert not f.any(), name
