"""Checked hoisted rotations on the GPU: clean calls return fhe_rotate_hoisted's words bit for bit (and the oracle composite's) with
every flag zero from a garbage-filled buffer; one armed bit flip in a shared stage raises exactly that shared word and changes every
rotation, one in a rotation's own stages -- the Galois permutation among them -- raises exactly that word of that rotation's block
and leaves the other rotations alone; the scope limits are error statuses."""
import ctypes as C

import numpy as np
import pytest

from helpers.checked_plan import checked_plan

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
PRODUCT, QUOTIENT, RESULT, SUM = 0, 1, 2, 3
WORD, INDEX = 0, 1
SHARED = ("intt_in", "extend", "ntt_ext")
ROT = ("mac", "galois", "intt_special", "moddown", "ntt_conv", "tail")      # execution order
STAGE_NAME = {0: "intt_in", 1: "extend", 2: "ntt_ext", 3: "mac", 8: "galois", 4: "intt_special", 5: "moddown", 6: "ntt_conv", 7: "tail"}


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


def _setup(F, eng, logn, L, K, dnum, kind, seed, n_keys):
    N = 1 << logn
    qs, t, ks, ab, rng = checked_plan(F, eng, logn, L, K, dnum, kind, seed)
    poly = lambda: np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs[:L]])
    c0, c1 = poly(), poly()
    keys = [np.stack([np.stack([np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs]) for _ in range(2)]) for _ in range(dnum)])
            for _ in range(n_keys)]
    return qs, t, ks, ab, c0, c1, keys


def _clean(flags, n_rot):
    assert sorted(flags["shared"]) == sorted(SHARED) and len(flags["rot"]) == n_rot
    for name, f in flags["shared"].items():
        assert not f.any(), f"shared stage {name}: flags {np.argwhere(f != 0).tolist()} = {f[f != 0].tolist()} on a clean run"
    for r, block in enumerate(flags["rot"]):
        assert sorted(block) == sorted(ROT)
        for name, f in block.items():
            assert not f.any(), f"rotation {r} stage {name}: flags {np.argwhere(f != 0).tolist()} = {f[f != 0].tolist()} on a clean run"


def _words(outs):
    return [(o0.download(), o1.download()) for o0, o1 in outs]


CLEAN = [(5, 3, 1, 3, "50"), (10, 4, 2, 2, "mixed"), (12, 6, 2, 3, "61"), (13, 4, 1, 4, "50/50"), (13, 5, 2, 1, "mixed"), (14, 3, 1, 3, "61")]


@pytest.mark.parametrize("logn,L,K,dnum,kind", CLEAN)
def test_clean_calls_return_the_unchecked_words_and_no_flag(F, eng, logn, L, K, dnum, kind):
    import torch
    from oracle.keyswitch_ref import rotate_hoisted_ref
    N, M = 1 << logn, L + K
    qs, t, ks, ab, c0, c1, keys = _setup(F, eng, logn, L, K, dnum, kind, logn * 31 + L * 5 + dnum, 5)
    d0, d1 = eng.upload(c0), eng.upload(c1)
    elts5 = [3, 5, 25, 2 * N - 1, 5]
    prepared5 = [ks.prepare_galois_key(eng.upload(key), k) for key, k in zip(keys, elts5)]
    # (rotation indices into elts5 / keys)
    batches = {1: [3], 2: [2, 0], 5: [0, 1, 2, 3, 4]}
    user = torch.cuda.Stream()
    for n_rot, idx in batches.items():
        elts, prepared = [elts5[i] for i in idx], [prepared5[i] for i in idx]
        lay = ks.rotate_hoisted_checked_layout(n_rot)
        per_rot = 2 * M + (2 * M + L) + 2 * K + 2 * (K + L) + 2 * L + 2 * L
        assert lay["shared_words"] == L + 2 * dnum * M and lay["rot_words"] == per_rot and lay["total"] == L + 2 * dnum * M + n_rot * per_rot
        assert [lay["shared"][s][0] for s in SHARED] == [0, L, L + dnum * M]
        assert [lay["rot"][s][0] for s in ROT] == list(np.cumsum([0, 2 * M, 2 * M + L, 2 * K, 2 * (K + L), 2 * L]))
        assert lay["rot"]["galois"][1] == (2 * M + L,)
        want = _words(ks.rotate_hoisted(d0, d1, elts, prepared))
        for stream in (None, C.c_void_p(user.cuda_stream)):
            outs, flags = ks.rotate_hoisted_checked(d0, d1, elts, prepared, ab, stream=stream)
            _clean(flags, n_rot)
            for r, (got, w) in enumerate(zip(_words(outs), want)):
                assert (got[0] == w[0]).all() and (got[1] == w[1]).all(), f"n_rot {n_rot} rotation {r} (element {elts[r]})"
            if stream is None and n_rot == 2 and logn <= 12:
                for r, (got, i) in enumerate(zip(_words(outs), idx)):
                    w0, w1 = rotate_hoisted_ref(c0, c1, elts5[i], keys[i], qs, L, K, dnum, logn)
                    assert (got[0] == w0).all() and (got[1] == w1).all(), f"oracle, rotation {r}"
        assert (d0.download() == c0).all() and (d1.download() == c1).all()          # inputs untouched
    eng.check()


def _expect_exactly(flags, n_rot, rot, stage, unit, what):
    """exactly the word (rot, stage, unit) is raised; rot is None for a shared stage"""
    for s, name in ((0, "intt_in"), (1, "extend"), (2, "ntt_ext")):
        hit = np.flatnonzero(flags["shared"][name].reshape(-1)).tolist()
        assert hit == ([unit] if rot is None and s == stage else []), f"{what}: shared stage {s} raised {hit}"
    for r in range(n_rot):
        for s in (3, 8, 4, 5, 6, 7):
            hit = np.flatnonzero(flags["rot"][r][STAGE_NAME[s]].reshape(-1)).tolist()
            assert hit == ([unit] if r == rot and s == stage else []), f"{what}: rotation {r} stage {s} raised {hit}"


def test_one_flip_raises_exactly_its_own_word(F, eng):
    from fhe_reliability_gpu_amd._lib import check, lib
    logn, L, K, dnum, n_rot = 13, 4, 2, 2, 3
    N, M, alpha = 1 << logn, L + K, 2
    qs, t, ks, ab, c0, c1, keys = _setup(F, eng, logn, L, K, dnum, "mixed", 77, n_rot)
    d0, d1 = eng.upload(c0), eng.upload(c1)
    elts = [3, 25, 2 * N - 1]
    prepared = [ks.prepare_galois_key(eng.upload(key), k) for key, k in zip(keys, elts)]
    run = lambda: ks.rotate_hoisted_checked(d0, d1, elts, prepared, ab)
    outs, flags = run()
    _clean(flags, n_rot)
    want = _words(outs)
    same = lambda got, r: (got[r][0] == want[r][0]).all() and (got[r][1] == want[r][1]).all()
    # (rot, stage, point, unit, coeff, bit); bit 30 of a word in flight always changes it and leaves it canonical for the next stage
    shared = [(0, 0, 0, 1, 5, 30), (0, 1, RESULT, M + alpha + 1, N - 1, 30), (2, 2, 0, alpha, N // 2 + 7, 30)]
    own = [(1, 3, PRODUCT, M + 1, 9, 30), (1, 4, 0, K, N - 1, 30), (1, 5, RESULT, (K + L) + 1, 77, 30), (1, 6, 0, L + 1, 0, 30), (1, 7, SUM, 0, 4097, 30),
           (1, 8, WORD, 1, 33, 30),                # a ciphertext row of half 0 of the sums
           (1, 8, WORD, M + L, N - 2, 30),         # the first special row of half 1
           (1, 8, WORD, 2 * M + 2, 1234, 30),      # row 2 of c0
           (1, 8, INDEX, M + 2, 4321, 4)]          # a wrong source index on a ciphertext row of half 1
    n = 0
    for rot, stage, point, unit, coeff, bit in shared + own:
        what = f"rotation {rot} stage {stage} point {point} unit {unit}"
        check(lib.fhe_ctx_inject_fault_rotate_hoisted(eng._h, rot, stage, point, unit, coeff, bit))
        outs, flags = run()
        got = _words(outs)
        if stage < 3:
            _expect_exactly(flags, n_rot, None, stage, unit, what)
            for r in range(n_rot):
                assert not same(got, r), f"{what}: rotation {r} unchanged"
        else:
            _expect_exactly(flags, n_rot, rot, stage, unit, what)
            assert not same(got, 1), f"{what}: rotation 1 unchanged"
            assert same(got, 0) and same(got, 2), f"{what}: another rotation changed"
        # one shot: the next call is clean again
        outs, flags = run()
        _clean(flags, n_rot)
        got = _words(outs)
        assert all(same(got, r) for r in range(n_rot))
        n += 1
    assert n == 12         # no case skipped
    eng.check()


def test_scope_limits_are_error_statuses(F, eng):
    from fhe_reliability_gpu_amd._lib import check, lib, vp
    logn, L, K, dnum, n_rot = 10, 4, 2, 2, 2
    N, M = 1 << logn, L + K
    qs, t, ks, ab, c0, c1, keys = _setup(F, eng, logn, L, K, dnum, "50", 3, n_rot)
    d0, d1 = eng.upload(c0), eng.upload(c1)
    elts = [3, 5]
    prepared = [ks.prepare_galois_key(eng.upload(key), k) for key, k in zip(keys, elts)]
    outs = [(eng.alloc(L * N), eng.alloc(L * N)) for _ in range(n_rot)]
    total = ks.rotate_hoisted_checked_layout(n_rot)["total"]
    fl = eng.upload(np.full((total + 1) // 2, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))
    ge = (C.c_uint32 * n_rot)(*elts)
    pk = (vp * n_rot)(*[k.ptr for k in prepared])

    def call(plan=None, abft=None, flags=fl.ptr, o0=None, n=n_rot, ge=ge):
        a0 = (vp * n_rot)(*(o0 or [o[0].ptr for o in outs]))
        a1 = (vp * n_rot)(*[o[1].ptr for o in outs])
        return lib.fhe_rotate_hoisted_checked(eng._h, plan or ks._h, a0, a1, d0.ptr, d1.ptr, ge, pk, n, abft or ab._h, flags, None)

    def clean_run():
        o, flags = ks.rotate_hoisted_checked(d0, d1, elts, prepared, ab)
        _clean(flags, n_rot)
        return o

    # no rotation: nothing launched, the flag buffer untouched
    assert call(n=0) == 0
    eng.sync()
    assert (fl.download() == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
    assert call() == 0
    want = _words(clean_run())
    # a sharded plan (one rank with gather buffers runs the phase path)
    g1, g2 = eng.alloc(L * N), eng.alloc(2 * K * N)
    sh = vp()
    check(lib.fhe_keyswitch_create_sharded(eng._h, t._h, L, K, dnum, 1, 0, g1.ptr, g2.ptr, None, C.byref(sh)))
    try:
        assert call(plan=sh) == INVALID
    finally:
        lib.fhe_keyswitch_destroy(sh)
    # a plan with a plain modulus
    ks.set_plain_modulus(65537)
    try:
        assert call() == UNSUPPORTED
    finally:
        ks.set_plain_modulus(0)
    # the fused transform
    eng.set_option("ntt_mode", 1)
    try:
        assert call() == UNSUPPORTED
    finally:
        eng.set_option("ntt_mode", 0)
    # a detector of another table set; null flags
    ab2 = F.Abft(eng, eng.tables(logn, qs))
    assert call(abft=ab2._h) == INVALID
    assert call(flags=None) == INVALID
    # an output aliasing c0; an even element
    assert call(o0=[outs[0][0].ptr, d0.ptr]) == INVALID
    assert call(ge=(C.c_uint32 * n_rot)(3, 4)) == INVALID
    # a rotation outside the call (stages 3-8 only: the shared stages ignore it)
    for stage, point in ((3, RESULT), (8, WORD)):
        check(lib.fhe_ctx_inject_fault_rotate_hoisted(eng._h, n_rot, stage, point, 0, 0, 30))
        assert call() == INVALID
    check(lib.fhe_ctx_inject_fault_rotate_hoisted(eng._h, 99, 1, RESULT, 0, 0, 30))
    o, flags = ks.rotate_hoisted_checked(d0, d1, elts, prepared, ab)
    _expect_exactly(flags, n_rot, None, 1, 0, "shared stage 1 with rot = 99")
    # the transform stages' hook needs a two-launch size: refused, nothing launched, nothing left armed
    for stage in (0, 2, 4, 6):
        check(lib.fhe_ctx_inject_fault_rotate_hoisted(eng._h, 0, stage, 0, 0 if stage != 2 else L // dnum, 5, 30))
        assert call() == UNSUPPORTED
        clean_run()
    # units, coefficients and points outside the call
    for stage, point, unit, coeff, bit, status in ((3, RESULT, 2 * M, 0, 30, INVALID), (8, WORD, 2 * M + L, 0, 30, INVALID), (8, WORD, 0, N, 30, INVALID),
                                                   (8, INDEX, 0, 0, logn, INVALID), (7, SUM, L, 0, 30, UNSUPPORTED), (5, SUM, 0, 0, 30, UNSUPPORTED)):
        check(lib.fhe_ctx_inject_fault_rotate_hoisted(eng._h, 1, stage, point, unit, coeff, bit))
        assert call() == status, (stage, point, unit, coeff, bit)
        clean_run()
    assert lib.fhe_ctx_inject_fault_rotate_hoisted(eng._h, 0, 9, 0, 0, 0, 0) == INVALID
    assert lib.fhe_ctx_inject_fault_rotate_hoisted(eng._h, 0, 8, 2, 0, 0, 0) == INVALID
    assert lib.fhe_ctx_inject_fault_rotate_hoisted(eng._h, -1, 3, 0, 0, 0, 0) == INVALID
    # the call neither takes nor honours the other hooks: an armed key-switch hook stays armed for the checked key switch
    check(lib.fhe_ctx_inject_fault_keyswitch(eng._h, 3, RESULT, 0, 0, 30))
    got = _words(clean_run())
    assert all((g[0] == w[0]).all() and (g[1] == w[1]).all() for g, w in zip(got, want))
    check(lib.fhe_ctx_inject_fault_keyswitch(eng._h, -1, 0, 0, 0, 0))
    eng.check()


def test_config5_hoisted_rotations_match_fhe_rotate_hoisted():
    """N = 2^16, L = 44, K = 11, dnum = 4 (BASELINE config 5), two rotations, on a sample of limbs."""
    import fhe_reliability_gpu_amd as F
    eng = F.default_engine()
    logn, L, K, dnum = 16, 44, 11, 4
    N = 1 << logn
    qs = F.create_moduli(N, [50] * L + [61] * K)
    t = eng.tables(logn, qs)
    ks, ab = F.KeySwitch(eng, t, L, K, dnum), F.Abft(eng, t)
    rng = np.random.default_rng(5)
    up = lambda *shape: eng.upload(rng.integers(0, min(qs), shape, dtype=np.uint64))
    c0, c1 = up(L, N), up(L, N)
    elts = [5, 2 * N - 1]
    prepared = [ks.prepare_galois_key(up(dnum, 2, L + K, N), k) for k in elts]
    outs, flags = ks.rotate_hoisted_checked(c0, c1, elts, prepared, ab)
    _clean(flags, 2)
    ref = ks.rotate_hoisted(c0, c1, elts, prepared)
    for r in range(2):
        for part in range(2):
            got, want = outs[r][part].download(), ref[r][part].download()
            for limb in (0, 1, 10, 11, 21, 33, 43):
                assert (got[limb] == want[limb]).all(), (r, part, limb)
    eng.check()
