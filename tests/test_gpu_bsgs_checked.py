"""Checked BSGS matrix-vector product and checked modular add on the GPU: clean calls return fhe_bsgs_matvec's words bit for bit (and
the oracle composite's) with every flag zero from a garbage-filled buffer; one armed bit flip -- in the inner sum, the accumulate,
or through one of the delegated hooks -- raises exactly its own word of the whole buffer and changes the output it fed; a diagonal
word >= q raises bit 4 alone; the scope limits are error statuses."""
import ctypes as C

import numpy as np
import pytest

from helpers.checked_plan import checked_plan

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
PRODUCT, QUOTIENT, RESULT, SUM = 0, 1, 2, 3
WORD = 0
KS_STAGES = ("intt_in", "extend", "ntt_ext", "mac", "intt_special", "moddown", "ntt_conv", "tail")
ROT_STAGES = ("mac", "galois", "intt_special", "moddown", "ntt_conv", "tail")


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


class _Case:
    def __init__(self, F, eng, logn, L, K, dnum, n1, n2, kind, seed):
        self.eng, self.logn, self.L, self.K, self.dnum, self.n1, self.n2 = eng, logn, L, K, dnum, n1, n2
        N = self.N = 1 << logn
        qs, self.t, self.ks, self.ab, rng = checked_plan(F, eng, logn, L, K, dnum, kind, seed)
        self.qs = qs
        mk = lambda rows: np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs[:rows]])
        key = lambda: np.stack([np.stack([mk(L + K) for _ in range(2)]) for _ in range(dnum)])
        self.c0, self.c1 = mk(L), mk(L)
        self.diags = np.stack([np.stack([mk(L) for _ in range(n1)]) for _ in range(n2)])
        self.baby_elts = [pow(3, b, 2 * N) for b in range(1, n1)]
        self.giant_elts = [pow(3, g * n1, 2 * N) for g in range(1, n2)]
        self.baby_keys, self.giant_keys = [key() for _ in self.baby_elts], [key() for _ in self.giant_elts]
        self.prepared = [self.ks.prepare_galois_key(eng.upload(k), e) for k, e in zip(self.baby_keys, self.baby_elts)]
        self.d_giant = [eng.upload(k) for k in self.giant_keys]
        self.d0, self.d1, self.dd = eng.upload(self.c0), eng.upload(self.c1), eng.upload(self.diags)

    def checked(self, diags=None, stream=None):
        o0, o1, fl = self.ks.bsgs_matvec_checked(self.d0, self.d1, diags or self.dd, self.n1, self.n2, self.baby_elts, self.prepared, self.giant_elts,
                                                 self.d_giant, self.ab, stream=stream)
        return o0.download(), o1.download(), fl

    def plain(self, diags=None):
        o0, o1 = self.ks.bsgs_matvec(self.d0, self.d1, diags or self.dd, self.n1, self.n2, self.baby_elts, self.prepared, self.giant_elts, self.d_giant)
        return o0.download(), o1.download()


def _raised(fl):
    """every non-zero flag word of the whole buffer as {(block, ..., stage, flat unit): value}"""
    out = {}

    def take(prefix, stages):
        for name, f in stages.items():
            for u in np.flatnonzero(f.reshape(-1)).tolist():
                out[prefix + (name, u)] = int(f.reshape(-1)[u])
    if fl["baby"] is not None:
        take(("baby", "shared"), fl["baby"]["shared"])
        for r, block in enumerate(fl["baby"]["rot"]):
            assert sorted(block) == sorted(ROT_STAGES)
            take(("baby", r), block)
    for g, block in enumerate(fl["giant"]):
        assert sorted(block) == ["acc", "galois", "inner", "keyswitch"] and sorted(block["keyswitch"]) == sorted(KS_STAGES)
        take(("giant", g), {k: v for k, v in block.items() if k != "keyswitch"})
        take(("giant", g, "keyswitch"), block["keyswitch"])
    return out


CLEAN = [(10, 3, 1, 3, 3, 2, "50/50"), (13, 4, 2, 2, 2, 3, "mixed"), (12, 3, 1, 1, 4, 1, "61"), (13, 3, 1, 3, 1, 2, "50"), (8, 2, 1, 2, 9, 2, "mixed"),
         (8, 2, 1, 1, 17, 2, "mixed"), (5, 2, 1, 2, 2, 2, "50")]


@pytest.mark.parametrize("logn,L,K,dnum,n1,n2,kind", CLEAN)
def test_clean_calls_return_the_unchecked_words_and_no_flag(F, eng, logn, L, K, dnum, n1, n2, kind):
    import torch
    from oracle.keyswitch_ref import bsgs_matvec_ref
    c = _Case(F, eng, logn, L, K, dnum, n1, n2, kind, logn * 31 + n1 * 7 + n2)
    M = L + K
    lay = c.ks.bsgs_matvec_checked_layout(n1, n2)
    ks_total = L + 2 * dnum * M + 2 * M + 2 * K + 2 * (K + L) + 2 * L + 2 * L
    per_rot = 2 * M + (2 * M + L) + 2 * K + 2 * (K + L) + 2 * L + 2 * L
    baby = 0 if n1 == 1 else L + 2 * dnum * M + (n1 - 1) * per_rot
    assert c.ks.checked_layout()["total"] == ks_total
    assert lay["baby"] == 0 and lay["baby_words"] == baby == lay["giant0"] and lay["giant_words"] == 5 * L + ks_total
    assert [lay["giant"][s][0] for s in ("inner", "galois", "acc", "keyswitch")] == [0, 2 * L, 4 * L, 5 * L]
    assert lay["total"] == baby + n2 * (5 * L + ks_total)
    if n1 > 1:
        assert c.ks.rotate_hoisted_checked_layout(n1 - 1)["total"] == baby
    want = c.plain()
    user = torch.cuda.Stream()
    for stream in (None, C.c_void_p(user.cuda_stream)):
        o0, o1, fl = c.checked(stream=stream)
        assert (fl["baby"] is None) == (n1 == 1) and len(fl["giant"]) == n2
        assert _raised(fl) == {}, "flags on a clean run"
        assert (o0 == want[0]).all() and (o1 == want[1]).all()
    if logn <= 12:
        w0, w1 = bsgs_matvec_ref(c.c0, c.c1, c.diags, c.baby_elts, c.baby_keys, c.giant_elts, c.giant_keys, c.qs, L, K, dnum, logn)
        assert (o0 == w0).all() and (o1 == w1).all(), "oracle"
    assert (c.d0.download() == c.c0).all() and (c.d1.download() == c.c1).all() and (c.dd.download() == c.diags).all()      # inputs untouched
    eng.check()


def _layout_refusals(c):
    from fhe_reliability_gpu_amd._lib import lib
    out = (C.c_int * 8)()
    for n1, n2 in ((0, 1), (1, 0), (4097, 1), (1, 4097)):
        assert lib.fhe_bsgs_matvec_checked_layout(c.ks._h, n1, n2, out) == INVALID
    assert lib.fhe_bsgs_matvec_checked_layout(c.ks._h, 4096, 4096, out) == 0


def _f64_final_quotient(q, ds, ys):
    """the quotient estimate of the final reduction of KsMacF64's running sum (fewer than eight terms: no fold), with Python's
    IEEE doubles and exact integers: each term is d y - rint(d (y / q)) q, exactly"""
    ninv = 1.0 / float(q)
    s = 0
    for d, y in zip(ds, ys):
        s += d * y - round(float(d) * (float(y) * ninv)) * q
    return round(float(s) * ninv)


def test_one_flip_raises_exactly_its_own_word(F, eng):
    from fhe_reliability_gpu_amd._lib import check, lib
    logn, L, K, dnum, n1, n2 = 13, 4, 2, 2, 3, 3
    c = _Case(F, eng, logn, L, K, dnum, n1, n2, "mixed", 77)
    N, M = c.N, L + K
    _layout_refusals(c)
    o0, o1, fl = c.checked()
    assert _raised(fl) == {}
    want = (o0, o1)
    assert all((g == w).all() for g, w in zip(c.plain(), want))
    # the words the inner sums read: part h of sigma_b(x), b = 0 the input itself (the checked words are the unchecked call's)
    rots = [(c.c0, c.c1)] + [(r0.download(), r1.download()) for r0, r1 in c.ks.rotate_hoisted(c.d0, c.d1, c.baby_elts, c.prepared)]
    F64, U64 = 0, 1          # limb 0 is a 50-bit prime (FP64 terms), limb 1 a 61-bit prime (Barrett)
    assert c.qs[F64] < 2**50 < c.qs[U64] and 2**61 - c.qs[U64] < 2**40

    def changed(got):
        return (got[0] != want[0]).any(), (got[1] != want[1]).any()

    def run(expect, feeds, what):
        got = c.checked()
        raised = _raised(got[2])
        assert list(raised) == [expect], f"{what}: raised {raised}"
        assert changed(got) == feeds, f"{what}: outputs changed {changed(got)}, expected {feeds}"
        # one shot: the next call is clean again
        got = c.checked()
        assert _raised(got[2]) == {} and changed(got) == (False, False), f"{what}: the call after it"

    n = 0
    # ---- inner sum: all four points, both parts, an FP64 limb and a U64 limb, g = 0 and g = 2.  Every flip is chosen so that the
    # wrong word is still canonical (a word >= q would, correctly, raise bit 4 where the next stage reads it):
    #   U64  product / sum / word: bit 30 moves the word by 2^30.  Quotient: q = 2^61 - e with e < 2^40, so bit 3 moves the 64-bit
    #        remainder by 8 q = -8 e (mod 2^64) and the word by 8 e
    #   FP64 product: bit 0 of h is one ulp, about 2^46 < q.  Sum / word: bit 30.  Quotient: bit 12 of a non-zero k scales it by
    #        1 + 2^-40, which moves the value by about 2^10 |k|; the coefficient is the first whose k is not 0 (a flip of a
    #        zero's mantissa is a denormal and changes nothing, which the CPU emulation covers)
    bits = {(U64, PRODUCT): 30, (U64, QUOTIENT): 3, (U64, RESULT): 30, (U64, SUM): 30,
            (F64, PRODUCT): 0, (F64, QUOTIENT): 12, (F64, RESULT): 30, (F64, SUM): 30}
    for g in (0, 2):
        for part in (0, 1):
            for limb in (F64, U64):
                for point in (PRODUCT, QUOTIENT, RESULT, SUM):
                    coeff = (1237 * (n + 1)) % N
                    if limb == F64 and point == QUOTIENT:
                        q = c.qs[limb]
                        while _f64_final_quotient(q, [int(c.diags[g, b, limb, coeff]) for b in range(n1)], [int(rots[b][part][limb, coeff]) for b in range(n1)]) == 0:
                            coeff += 1
                    unit = part * L + limb
                    check(lib.fhe_ctx_inject_fault_bsgs(eng._h, g, 0, point, unit, coeff, bits[limb, point]))
                    # g = 0 writes the outputs themselves; g >= 1: part 0 is added to out0, part 1 goes through the key switch
                    feeds = (part == 0, part == 1) if g == 0 or part == 0 else (True, True)
                    run(("giant", g, "inner", unit), feeds, f"inner sum g {g} part {part} limb {limb} point {point} coeff {coeff}")
                    n += 1
    assert n == 32
    # ---- accumulate: the word and the sum, g = 1 and g = 2; it feeds out0 alone
    for g, point, limb in ((1, RESULT, F64), (1, SUM, U64), (2, SUM, F64), (2, RESULT, U64)):
        check(lib.fhe_ctx_inject_fault_bsgs(eng._h, g, 1, point, limb, 4097 + g, 30))
        run(("giant", g, "acc", limb), (True, False), f"accumulate g {g} point {point} limb {limb}")
    # ---- the delegated hooks, each in its own step
    check(lib.fhe_ctx_inject_fault_rotate_hoisted(eng._h, 1, 3, PRODUCT, M + 1, 9, 30))        # baby rotation 1, stage 3, half 1 row 1 (U64)
    run(("baby", 1, "mac", M + 1), (True, True), "baby block stage 3")
    check(lib.fhe_ctx_inject_fault_galois(eng._h, WORD, 1, 33, 30))                             # g = 1, row 1 of part 0
    run(("giant", 1, "galois", 1), (True, False), "Galois permutation at g = 1")
    check(lib.fhe_ctx_inject_fault_keyswitch(eng._h, 7, SUM, L + 1, 4097, 30))                  # g = 1, tail, half 1 (addend out1)
    run(("giant", 1, "keyswitch", "tail", L + 1), (False, True), "key switch stage 7 point 3 at g = 1")
    check(lib.fhe_ctx_inject_fault_keyswitch(eng._h, 7, SUM, 0, 5, 30))                         # half 0 (addend t0)
    run(("giant", 1, "keyswitch", "tail", 0), (True, False), "key switch stage 7 point 3 at g = 1, half 0")
    eng.check()


def test_a_diagonal_word_out_of_range_raises_bit_4_alone_on_both_parts(F, eng):
    logn, L, K, dnum, n1, n2 = 10, 3, 1, 3, 3, 2
    c = _Case(F, eng, logn, L, K, dnum, n1, n2, "mixed", 4)
    for g, b, limb, coeff, over in ((0, 0, 0, 5, 0), (1, 2, 1, c.N - 1, 12345), (1, 1, 2, 77, 2**63)):
        diags = c.diags.copy()
        diags[g, b, limb, coeff] = np.uint64(c.qs[limb] + over)
        dd = eng.upload(diags)
        o0, o1, fl = c.checked(diags=dd)
        assert _raised(fl) == {("giant", g, "inner", limb): 4, ("giant", g, "inner", L + limb): 4}
        w0, w1 = c.plain(diags=dd)
        assert (o0 == w0).all() and (o1 == w1).all()
    eng.check()


def test_scope_limits_are_error_statuses(F, eng):
    from fhe_reliability_gpu_amd._lib import check, lib, vp
    logn, L, K, dnum, n1, n2 = 10, 3, 1, 3, 2, 2
    c = _Case(F, eng, logn, L, K, dnum, n1, n2, "50", 3)
    N = c.N
    o0, o1 = eng.alloc(L * N), eng.alloc(L * N)
    total = c.ks.bsgs_matvec_checked_layout(n1, n2)["total"]
    fl = eng.upload(np.full((total + 1) // 2, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))
    be, ge = (C.c_uint32 * 1)(*c.baby_elts), (C.c_uint32 * 1)(*c.giant_elts)
    bk, gk = (vp * 1)(c.prepared[0].ptr), (vp * 1)(c.d_giant[0].ptr)

    def call(plan=None, abft=None, out0=None, n1_=n1, n2_=n2):
        return lib.fhe_bsgs_matvec_checked(eng._h, plan or c.ks._h, out0 or o0.ptr, o1.ptr, c.d0.ptr, c.d1.ptr, c.dd.ptr, n1_, n2_, be, bk, ge, gk,
                                           abft or c.ab._h, fl.ptr, None)

    want = c.plain()

    def clean_run():
        g0, g1, flags = c.checked()
        assert _raised(flags) == {} and (g0 == want[0]).all() and (g1 == want[1]).all()

    assert call() == 0
    clean_run()
    # a sharded plan (one rank with gather buffers runs the phase path)
    g1b, g2b = eng.alloc(L * N), eng.alloc(2 * K * N)
    sh = vp()
    check(lib.fhe_keyswitch_create_sharded(eng._h, c.t._h, L, K, dnum, 1, 0, g1b.ptr, g2b.ptr, None, C.byref(sh)))
    try:
        assert call(plan=sh) == INVALID
    finally:
        lib.fhe_keyswitch_destroy(sh)
    # a plan with a plain modulus
    c.ks.set_plain_modulus(65537)
    try:
        assert call() == UNSUPPORTED
    finally:
        c.ks.set_plain_modulus(0)
    # in-place arguments; a detector made for another table set; shapes outside the limits
    assert call(out0=c.d0.ptr) == INVALID
    assert call(out0=o1.ptr) == INVALID
    t2 = eng.tables(logn, c.qs)
    ab2 = F.Abft(eng, t2)
    assert call(abft=ab2._h) == INVALID
    assert call(n1_=0) == INVALID and call(n2_=4097) == INVALID
    clean_run()
    # the hook outside the call, stage 1 at g = 0, points 0 and 1 on the add: refused, nothing launched, the hook used up
    refusals = [((n2, 0, RESULT, 0, 0, 30), INVALID), ((0, 0, RESULT, 2 * L, 0, 30), INVALID), ((1, 0, RESULT, 0, N, 30), INVALID),
                ((1, 1, RESULT, L, 0, 30), INVALID), ((0, 1, RESULT, 0, 0, 30), INVALID), ((1, 1, PRODUCT, 0, 0, 30), UNSUPPORTED),
                ((1, 1, QUOTIENT, 0, 0, 30), UNSUPPORTED)]
    for args, status in refusals:
        check(lib.fhe_ctx_inject_fault_bsgs(eng._h, *args))
        check(lib.fhe_memset(eng._h, fl.ptr, 0xA5, ((total + 1) // 2) * 8, None))
        assert call() == status, args
        eng.sync()
        assert (fl.download() == np.uint64(0xA5A5A5A5A5A5A5A5)).all(), f"{args}: something was launched"
        clean_run()
    # a delegated hook whose fault lies outside its step, or whose step the call does not have
    check(lib.fhe_ctx_inject_fault_galois(eng._h, WORD, 2 * L, 0, 30))
    assert call() == INVALID
    clean_run()
    check(lib.fhe_ctx_inject_fault_keyswitch(eng._h, 3, RESULT, 0, 0, 30))
    assert call(n2_=1) == INVALID
    clean_run()
    check(lib.fhe_ctx_inject_fault_rotate_hoisted(eng._h, 1, 3, RESULT, 0, 0, 30))      # one baby rotation: rot 1 is outside
    assert call() == INVALID
    clean_run()
    for bad in ((0, 2, 0, 0, 0, 0), (-1, 0, 0, 0, 0, 0), (0, 0, 4, 0, 0, 0), (0, 0, 0, -1, 0, 0), (0, 0, 0, 0, -1, 0), (0, 0, 0, 0, 0, 64)):
        assert lib.fhe_ctx_inject_fault_bsgs(eng._h, *bad) == INVALID
    check(lib.fhe_ctx_inject_fault_bsgs(eng._h, 0, 0, RESULT, 0, 0, 30))
    check(lib.fhe_ctx_inject_fault_bsgs(eng._h, 0, -1, 0, 0, 0, 0))                      # cleared
    clean_run()
    eng.check()


def test_modadd_checked_equals_modadd_and_a_flip_raises_its_word(F, eng):
    from fhe_reliability_gpu_amd._lib import check, lib
    logn, n_poly, limbs = 6, 2, 3
    N = 1 << logn
    qs = F.create_moduli(N, [50, 61, 50])
    t = eng.tables(logn, qs)
    rng = np.random.default_rng(6)
    mk = lambda: np.stack([np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs]) for _ in range(n_poly)])
    a, b = mk(), mk()
    a[0, 0, :3], b[0, 0, :3] = (0, 1, qs[0] - 1), (0, qs[0] - 1, qs[0] - 1)          # 0 + 0, a + b = q exactly, the largest sum
    da, db, dc, dw = eng.upload(a), eng.upload(b), eng.alloc(a.size), eng.alloc(a.size)
    check(lib.fhe_modadd(eng._h, dw.ptr, da.ptr, db.ptr, t._h, n_poly, limbs, 0, None))
    want = dw.download().reshape(a.shape)
    assert [int(v) for v in want[1, 1]] == [(int(x) + int(y)) % qs[1] for x, y in zip(a[1, 1], b[1, 1])]
    f = t.modadd_checked(dc, da, db, n_poly=n_poly)
    assert f.shape == (n_poly * limbs,) and not f.any() and (dc.download().reshape(a.shape) == want).all()
    # in place, c == a
    dai = eng.upload(a)
    f = t.modadd_checked(dai, dai, db, n_poly=n_poly)
    assert not f.any() and (dai.download().reshape(a.shape) == want).all()
    # one flip raises exactly its (poly, limb) word
    for point, poly, limb, coeff in ((RESULT, 0, 1, 0), (SUM, 1, 2, N - 1), (SUM, 0, 0, 2), (RESULT, 1, 0, 17)):
        check(lib.fhe_ctx_inject_fault_pointwise(eng._h, point, (poly * limbs + limb) * N + coeff, 30))
        f = t.modadd_checked(dc, da, db, n_poly=n_poly)
        assert np.flatnonzero(f).tolist() == [poly * limbs + limb], (point, poly, limb)
        got = dc.download().reshape(a.shape)
        diff = np.argwhere(got != want).tolist()
        assert diff == [[poly, limb, coeff]], (point, diff)
        f = t.modadd_checked(dc, da, db, n_poly=n_poly)                                # one shot
        assert not f.any() and (dc.download().reshape(a.shape) == want).all()
    # no product and no quotient estimate on an add; an index outside the window; a non-canonical operand
    fl = eng.alloc(n_poly * limbs)
    for point in (PRODUCT, QUOTIENT):
        check(lib.fhe_ctx_inject_fault_pointwise(eng._h, point, 0, 30))
        assert lib.fhe_modadd_checked(eng._h, dc.ptr, da.ptr, db.ptr, t._h, n_poly, limbs, 0, fl.ptr, None) == UNSUPPORTED
        assert not t.modadd_checked(dc, da, db, n_poly=n_poly).any()
    check(lib.fhe_ctx_inject_fault_pointwise(eng._h, RESULT, n_poly * limbs * N, 30))
    assert lib.fhe_modadd_checked(eng._h, dc.ptr, da.ptr, db.ptr, t._h, n_poly, limbs, 0, fl.ptr, None) == INVALID
    a2 = a.copy()
    a2[1, 2, 9] = np.uint64(qs[2] + 3)
    da2 = eng.upload(a2)
    f = t.modadd_checked(dc, da2, db, n_poly=n_poly)
    assert f.tolist() == [0, 0, 0, 0, 0, 4]
    check(lib.fhe_modadd(eng._h, dw.ptr, da2.ptr, db.ptr, t._h, n_poly, limbs, 0, None))
    assert (dc.download() == dw.download()).all()
    eng.check()
