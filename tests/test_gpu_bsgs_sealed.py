"""Sealed BSGS matrix-vector product on the GPU: clean calls return fhe_bsgs_matvec's words bit for bit (and the oracle composite's)
with every flag zero from a garbage-filled buffer and the outputs sealed; a word changed in memory after sealing -- in a diagonal,
in c1, in a key, in a seal -- raises exactly its own row's word and nothing in the checked block; a flip on the consuming load of
a diagonal raises its row while the residue identity holds on the wrong operand; the scope limits are error statuses with nothing
launched."""
import ctypes as C

import numpy as np
import pytest

from helpers.checked_plan import checked_plan

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
SEAL_SUM, SEAL_RANGE = 1, 2
P = (1 << 61) - 1
KS_STAGES = ("intt_in", "extend", "ntt_ext", "mac", "intt_special", "moddown", "ntt_conv", "tail")
ROT_STAGES = ("mac", "galois", "intt_special", "moddown", "ntt_conv", "tail")
INPUTS = ("c0", "c1", "baby_keys", "giant_keys", "diags")


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
        # the seals, taken once from the operands as they are now: the PREPARED baby keys, as the caller holds them
        self.seals = (self.t.seal(self.d0, limbs=L), self.t.seal(self.d1, limbs=L))
        self.baby_seals = [self.ks.seal_key(k) for k in self.prepared]
        self.giant_seals = [self.ks.seal_key(k) for k in self.d_giant]
        self.diag_seal = self.ks.seal_diagonals(self.dd, n1, n2)

    def sealed(self, stream=None, **over):
        a = dict(c0=self.d0, c1=self.d1, diags=self.dd, prepared=self.prepared, giant=self.d_giant, seals=self.seals, baby_seals=self.baby_seals,
                 giant_seals=self.giant_seals, diag_seal=self.diag_seal)
        a.update(over)
        o0, o1, so, fl = self.ks.bsgs_matvec_sealed(a["c0"], a["c1"], a["diags"], self.n1, self.n2, self.baby_elts, a["prepared"], self.giant_elts, a["giant"],
                                                    self.ab, seals=a["seals"], baby_key_seals=a["baby_seals"], giant_key_seals=a["giant_seals"],
                                                    diag_seal=a["diag_seal"], stream=stream)
        return o0.download(), o1.download(), so, fl

    def plain(self, **over):
        a = dict(c0=self.d0, c1=self.d1, diags=self.dd, prepared=self.prepared, giant=self.d_giant)
        a.update(over)
        o0, o1 = self.ks.bsgs_matvec(a["c0"], a["c1"], a["diags"], self.n1, self.n2, self.baby_elts, a["prepared"], self.giant_elts, a["giant"])
        return o0.download(), o1.download()


def _raised_checked(fl):
    """every non-zero flag word of the checked block as {(block, ..., stage, flat unit): value}"""
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


def _raised(fl):
    """every non-zero flag word of the whole buffer: input rows as {(name, index...): value}, the checked block under "checked" """
    assert sorted(fl) == sorted(INPUTS + ("checked",))
    out = {}
    for name in INPUTS:
        for idx in np.argwhere(fl[name]).tolist():
            out[(name,) + tuple(idx)] = int(fl[name][tuple(idx)])
    for k, v in _raised_checked(fl["checked"]).items():
        out[("checked",) + k] = v
    return out


def _sums(row):
    """{S0, S1} of one row, Python integers"""
    row = [int(v) for v in row]
    return [sum(row) % P, sum((j + 1) * v for j, v in enumerate(row)) % P]


# a row shorter than a workgroup; NB = 4 with one term; the edge of NB = 4; the first n1 of NB = 8 on two arithmetic paths; two chunks
# per row (the weight is the ROW index); the edge of NB = 8; the first n1 of NB = 16; its edge; the fallback route
CLEAN = [(5, 2, 1, 2, 2, 2, "50"), (10, 3, 1, 3, 1, 2, "mixed"), (10, 3, 1, 3, 4, 2, "50/50"), (13, 4, 2, 2, 5, 2, "mixed"), (14, 2, 1, 2, 3, 2, "61"),
         (8, 2, 1, 1, 8, 1, "mixed"), (8, 2, 1, 2, 9, 2, "mixed"), (8, 2, 1, 1, 16, 1, "mixed"), (8, 2, 1, 1, 17, 2, "mixed")]


@pytest.mark.parametrize("logn,L,K,dnum,n1,n2,kind", CLEAN)
def test_clean_calls_return_the_unchecked_words_sealed_and_no_flag(F, eng, logn, L, K, dnum, n1, n2, kind):
    import torch
    from oracle.keyswitch_ref import bsgs_matvec_ref
    c = _Case(F, eng, logn, L, K, dnum, n1, n2, kind, logn * 37 + n1 * 5 + n2)
    M = L + K
    kr = dnum * 2 * M
    lay = c.ks.bsgs_matvec_sealed_layout(n1, n2)
    inner = c.ks.bsgs_matvec_checked_layout(n1, n2)
    offs = [0, L, 2 * L, 2 * L + (n1 - 1) * kr, 2 * L + (n1 + n2 - 2) * kr, 2 * L + (n1 + n2 - 2) * kr + n2 * n1 * L]
    assert [lay[k][0] for k in INPUTS] + [lay["checked"]] == offs
    assert lay["total"] == offs[5] + inner["total"]
    assert lay["diags"][1] == (n2, n1, L) and lay["baby_keys"][1] == (n1 - 1, dnum, 2, M) and lay["giant_keys"][1] == (n2 - 1, dnum, 2, M)
    want = c.plain()
    user = torch.cuda.Stream()
    for stream in (None, C.c_void_p(user.cuda_stream)):
        o0, o1, so, fl = c.sealed(stream=stream)
        assert (fl["checked"]["baby"] is None) == (n1 == 1) and len(fl["checked"]["giant"]) == n2
        assert _raised(fl) == {}, "flags on a clean run"
        assert (o0 == want[0]).all() and (o1 == want[1]).all()
        # the outputs' seals: those of fhe_seal, and Python-integer sums of one row
        for h, o in enumerate((o0, o1)):
            got = so[h].download()
            assert (got == c.t.seal(eng.upload(o), limbs=L).download()).all()
            assert [int(v) for v in got[L - 1]] == _sums(o[L - 1])
    if logn <= 12:
        w0, w1 = bsgs_matvec_ref(c.c0, c.c1, c.diags, c.baby_elts, c.baby_keys, c.giant_elts, c.giant_keys, c.qs, L, K, dnum, logn)
        assert (o0 == w0).all() and (o1 == w1).all(), "oracle"
    assert (c.d0.download() == c.c0).all() and (c.d1.download() == c.c1).all() and (c.dd.download() == c.diags).all()      # inputs untouched
    # the stored seal of a diagonal row is fhe_seal's: Python-integer sums of the last row
    assert [int(v) for v in c.diag_seal.download()[n2 * n1 * L - 1]] == _sums(c.diags[n2 - 1, n1 - 1, L - 1])
    # without seals nothing is verified and nothing is raised
    o0, o1, so, fl = c.sealed(seals=None, baby_seals=None, giant_seals=None, diag_seal=None)
    assert _raised(fl) == {} and (o0 == want[0]).all() and (o1 == want[1]).all()
    eng.check()


def _one_row(c, expect, **over):
    """a call on corrupted memory: exactly `expect` raised, nothing in the checked block, the words bsgs_matvec's on that memory"""
    o0, o1, so, fl = c.sealed(**over)
    assert _raised(fl) == expect, _raised(fl)
    w0, w1 = c.plain(**{k: v for k, v in over.items() if k in ("c0", "c1", "diags", "prepared", "giant")})
    assert (o0 == w0).all() and (o1 == w1).all()
    return o0, o1


def test_a_word_changed_in_memory_after_sealing_raises_exactly_its_row(F, eng):
    logn, L, K, dnum, n1, n2 = 10, 3, 1, 3, 3, 2
    c = _Case(F, eng, logn, L, K, dnum, n1, n2, "mixed", 11)
    N, M = c.N, L + K
    want = c.plain()
    flip = lambda a, idx: a.__setitem__(idx, a[idx] ^ np.uint64(1 << 3))      # stays below q: q - 1 is a multiple of 2 N
    # diagonals: (g = 0, b = 0) and (g = last, b = last)
    for g, b, limb, j in ((0, 0, 1, 0), (n2 - 1, n1 - 1, L - 1, N - 1)):
        diags = c.diags.copy()
        flip(diags, (g, b, limb, j))
        assert int(diags[g, b, limb, j]) < c.qs[limb]
        o0, o1 = _one_row(c, {("diags", g, b, limb): SEAL_SUM}, diags=eng.upload(diags))
        assert (o0 != want[0]).any() or (o1 != want[1]).any()
    # c1
    c1 = c.c1.copy()
    flip(c1, (2, 77))
    _one_row(c, {("c1", 2): SEAL_SUM}, c1=eng.upload(c1))
    # a prepared baby key, as the caller holds it
    key = c.prepared[1].download().copy()
    flip(key, (dnum - 1, 1, M - 1, 5))
    dk = eng.upload(key)
    _one_row(c, {("baby_keys", 1, dnum - 1, 1, M - 1): SEAL_SUM}, prepared=[c.prepared[0], dk])
    # a giant key
    key = c.giant_keys[0].copy()
    flip(key, (0, 0, 1, N - 2))
    _one_row(c, {("giant_keys", 0, 0, 0, 1): SEAL_SUM}, giant=[eng.upload(key)])
    # a seal word of a diagonal row: the words are right, the row is raised
    seal = c.diag_seal.download().copy()
    row = (1 * n1 + 1) * L + 2
    seal[row, 1] ^= np.uint64(1 << 40)
    ds = eng.upload(seal)
    ds.shape = seal.shape
    o0, o1 = _one_row(c, {("diags", 1, 1, 2): SEAL_SUM}, diag_seal=ds)
    assert (o0 == want[0]).all() and (o1 == want[1]).all()
    eng.check()


def test_a_diagonal_word_in_the_second_chunk_is_weighted_by_its_row_index(F, eng):
    logn, L, K, dnum, n1, n2 = 14, 2, 1, 2, 3, 2
    c = _Case(F, eng, logn, L, K, dnum, n1, n2, "61", 5)
    # two words of the second chunk swapped with d1 = -d2: S0 does not move; S1 moves only if the weights are row indices that differ
    g, b, limb, j1, j2 = 1, 2, 1, (1 << 13) + 4, (1 << 13) + 4 + 255
    diags = c.diags.copy()
    d = min(1 << 20, int(diags[g, b, limb, j2]), c.qs[limb] - 1 - int(diags[g, b, limb, j1]))
    assert d > 0
    diags[g, b, limb, j1] += np.uint64(d)
    diags[g, b, limb, j2] -= np.uint64(d)
    assert _sums(diags[g, b, limb])[0] == _sums(c.diags[g, b, limb])[0]
    _one_row(c, {("diags", g, b, limb): SEAL_SUM}, diags=eng.upload(diags))
    # one word of the second chunk
    diags = c.diags.copy()
    diags[0, 1, 0, c.N - 1] ^= np.uint64(1 << 3)
    _one_row(c, {("diags", 0, 1, 0): SEAL_SUM}, diags=eng.upload(diags))
    eng.check()


def test_the_fallback_route_raises_the_same_word(F, eng):
    logn, L, K, dnum, n1, n2 = 8, 2, 1, 1, 17, 2
    c = _Case(F, eng, logn, L, K, dnum, n1, n2, "mixed", 13)
    for g, b, limb, j in ((0, 0, 0, 3), (1, 16, 1, c.N - 1)):
        diags = c.diags.copy()
        diags[g, b, limb, j] ^= np.uint64(1 << 3)
        _one_row(c, {("diags", g, b, limb): SEAL_SUM}, diags=eng.upload(diags))
    eng.check()


@pytest.mark.parametrize("n1", [3, 17])
def test_a_diagonal_word_out_of_range_raises_range_and_sum_and_bit_4_on_both_parts(F, eng, n1):
    logn, L, K, dnum, n2 = 8, 2, 1, 2, 2
    c = _Case(F, eng, logn, L, K, dnum, n1, n2, "mixed", 4)
    g, b, limb, j = 1, n1 - 1, 1, 9
    diags = c.diags.copy()
    diags[g, b, limb, j] = np.uint64(c.qs[limb] + 3)
    _one_row(c, {("diags", g, b, limb): SEAL_RANGE | SEAL_SUM, ("checked", "giant", g, "inner", limb): 4, ("checked", "giant", g, "inner", L + limb): 4},
             diags=eng.upload(diags))
    eng.check()


def _hook_on_the_consuming_load(F, eng, shape, seed, words):
    from fhe_reliability_gpu_amd._lib import check, lib
    logn, L, K, dnum, n1, n2 = shape
    c = _Case(F, eng, logn, L, K, dnum, n1, n2, "mixed", seed)
    want = c.plain()
    for g, b, limb, j in words:
        word = int(c.diags[g, b, limb, j])
        bit = max(i for i in range(61) if word >> i & 1)          # a bit that is SET: the flipped word stays below q
        assert word ^ (1 << bit) < c.qs[limb]
        check(lib.fhe_ctx_inject_fault_bsgs_sealed(eng._h, g, b, limb, j, bit))
        o0, o1, so, fl = c.sealed()
        # the gap shown: the residue identity holds on the wrong operand, the inner words stay zero
        assert _raised(fl) == {("diags", g, b, limb): SEAL_SUM}
        # memory stayed clean: the words are those of the product on the flipped diagonal
        diags = c.diags.copy()
        diags[g, b, limb, j] = np.uint64(word ^ (1 << bit))
        w0, w1 = c.plain(diags=eng.upload(diags))
        assert (o0 == w0).all() and (o1 == w1).all()
        if g == 0:                                               # written straight into the outputs: that limb, and no other
            others = [l for l in range(L) if l != limb]
            assert (o0[limb] != want[0][limb]).any() and (o0[others] == want[0][others]).all() and (o1[others] == want[1][others]).all()
        else:                                                    # through the permutation and the key switch
            assert (o0 != want[0]).any() and (o1 != want[1]).any()
        assert (c.dd.download() == c.diags).all()
        # one shot: the next call is clean
        o0, o1, so, fl = c.sealed()
        assert _raised(fl) == {} and (o0 == want[0]).all() and (o1 == want[1]).all()
    # a delegated hook of the checked body keeps working: the inner sum's own
    check(lib.fhe_ctx_inject_fault_bsgs(eng._h, 1, 0, 2, L + 1, 33, 30))
    o0, o1, so, fl = c.sealed()
    assert _raised(fl) == {("checked", "giant", 1, "inner", L + 1): 1}
    o0, o1, so, fl = c.sealed()
    assert _raised(fl) == {}
    eng.check()


def test_the_hook_on_the_consuming_load_raises_the_row_and_not_the_residue_check(F, eng):
    _hook_on_the_consuming_load(F, eng, (10, 3, 1, 3, 3, 2), 21, ((0, 0, 0, 0), (1, 2, 1, (1 << 10) - 1), (1, 1, 2, 513)))


def test_the_hook_on_the_consuming_load_at_sixteen_baby_steps(F, eng):
    """the hooked form of the widest instantiation: the first and the last diagonal of a giant step, and one between"""
    _hook_on_the_consuming_load(F, eng, (8, 2, 1, 1, 16, 2), 23, ((0, 0, 0, 0), (1, 15, 1, (1 << 8) - 1), (1, 7, 0, 129)))


def test_the_hook_on_the_fallback_route_lives_in_the_verifying_sweep(F, eng):
    from fhe_reliability_gpu_amd._lib import check, lib
    logn, L, K, dnum, n1, n2 = 8, 2, 1, 1, 17, 2
    c = _Case(F, eng, logn, L, K, dnum, n1, n2, "mixed", 22)
    want = c.plain()
    for g, b, limb, j in ((0, 16, 1, 7), (1, 0, 0, c.N - 1)):
        word = int(c.diags[g, b, limb, j])
        bit = max(i for i in range(61) if word >> i & 1)
        check(lib.fhe_ctx_inject_fault_bsgs_sealed(eng._h, g, b, limb, j, bit))
        o0, o1, so, fl = c.sealed()
        assert _raised(fl) == {("diags", g, b, limb): SEAL_SUM}
        assert (o0 == want[0]).all() and (o1 == want[1]).all()
        o0, o1, so, fl = c.sealed()
        assert _raised(fl) == {}
    eng.check()


def test_scope_limits_are_error_statuses_with_nothing_launched(F, eng):
    from fhe_reliability_gpu_amd._lib import check, lib, vp
    logn, L, K, dnum, n1, n2 = 10, 3, 1, 3, 2, 2
    c = _Case(F, eng, logn, L, K, dnum, n1, n2, "50", 3)
    N = c.N
    o0, o1 = eng.alloc(L * N), eng.alloc(L * N)
    so = [eng.alloc(2 * L), eng.alloc(2 * L)]
    total = c.ks.bsgs_matvec_sealed_layout(n1, n2)["total"]
    words = (total + 1) // 2
    fl = eng.upload(np.full(words, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))
    be, ge = (C.c_uint32 * 1)(*c.baby_elts), (C.c_uint32 * 1)(*c.giant_elts)
    bk, gk = (vp * 1)(c.prepared[0].ptr), (vp * 1)(c.d_giant[0].ptr)
    sin, sout = (vp * 2)(c.seals[0].ptr, c.seals[1].ptr), (vp * 2)(so[0].ptr, so[1].ptr)
    bs, gs = (vp * 1)(c.baby_seals[0].ptr), (vp * 1)(c.giant_seals[0].ptr)

    def call(plan=None, out0=None, diags=None, n1_=n1, n2_=n2, diag_seal=True):
        return lib.fhe_bsgs_matvec_sealed(eng._h, plan or c.ks._h, out0 or o0.ptr, o1.ptr, c.d0.ptr, c.d1.ptr, diags or c.dd.ptr, n1_, n2_, be, bk, ge, gk,
                                          c.ab._h, sin, bs, gs, c.diag_seal.ptr if diag_seal else None, sout, fl.ptr, None)

    want = c.plain()

    def clean_run():
        g0, g1, _, flags = c.sealed()
        assert _raised(flags) == {} and (g0 == want[0]).all() and (g1 == want[1]).all()

    def refused(status, what, **kw):
        check(lib.fhe_memset(eng._h, fl.ptr, 0xA5, words * 8, None))
        assert call(**kw) == status, what
        eng.sync()
        assert (fl.download() == np.uint64(0xA5A5A5A5A5A5A5A5)).all(), f"{what}: something was launched"

    assert call() == 0
    eng.sync()
    assert not fl.download().view(np.uint32)[:total].any()
    clean_run()
    # a sharded plan (one rank with gather buffers runs the phase path)
    g1b, g2b = eng.alloc(L * N), eng.alloc(2 * K * N)
    sh = vp()
    check(lib.fhe_keyswitch_create_sharded(eng._h, c.t._h, L, K, dnum, 1, 0, g1b.ptr, g2b.ptr, None, C.byref(sh)))
    try:
        refused(INVALID, "sharded plan", plan=sh)
    finally:
        lib.fhe_keyswitch_destroy(sh)
    # a plan with a plain modulus
    c.ks.set_plain_modulus(65537)
    try:
        refused(UNSUPPORTED, "plain modulus")
    finally:
        c.ks.set_plain_modulus(0)
    # a misaligned diagonal pointer; in-place outputs; shapes outside the limits
    refused(INVALID, "misaligned diagonals", diags=C.c_void_p(c.dd.ptr.value + 8))
    refused(INVALID, "in place", out0=c.d0.ptr)
    refused(INVALID, "out0 == out1", out0=o1.ptr)
    refused(INVALID, "n1 = 0", n1_=0)
    refused(INVALID, "n2 = 4097", n2_=4097)
    clean_run()
    # a hook outside the call: refused, nothing launched, the hook used up
    for args in ((n2, 0, 0, 0, 3), (0, n1, 0, 0, 3), (0, 0, L, 0, 3), (0, 0, 0, N, 3)):
        check(lib.fhe_ctx_inject_fault_bsgs_sealed(eng._h, *args))
        refused(INVALID, args)
        clean_run()
    check(lib.fhe_ctx_inject_fault_bsgs_sealed(eng._h, 0, 0, 0, 0, 3))
    refused(INVALID, "a hook without diagonal seals", diag_seal=False)
    clean_run()
    for bad in ((0, -1, 0, 0, 0), (0, 0, -1, 0, 0), (0, 0, 0, -1, 0), (0, 0, 0, 0, 64), (0, 0, 0, 0, -1)):
        assert lib.fhe_ctx_inject_fault_bsgs_sealed(eng._h, *bad) == INVALID
    check(lib.fhe_ctx_inject_fault_bsgs_sealed(eng._h, 0, 0, 0, 0, 3))
    check(lib.fhe_ctx_inject_fault_bsgs_sealed(eng._h, -1, 0, 0, 0, 0))                   # cleared
    clean_run()
    # the layout call's own refusals
    out = (C.c_int * 8)()
    for a, b in ((0, 1), (1, 0), (4097, 1), (1, 4097)):
        assert lib.fhe_bsgs_matvec_sealed_layout(c.ks._h, a, b, out) == INVALID
    assert lib.fhe_bsgs_matvec_sealed_layout(c.ks._h, 16, 16, out) == 0
    eng.check()
