"""The round-to-nearest rescale (fhe_keyswitch_set_rescale_rounding) on every launch list of the plan: the three-launch list
(2^4), the conversion's replacement plus the single-launch tail (2^8, 2^12), the centring on the column pass's load (2^13), the
fused multiply's second input and its unfused route, the sharded phases of both, and the refusals.  Every comparison of words is
== against tests/helpers/rescale_round.py, whose two statements of the definition tests/test_rescale_round_ref.py holds against each
other; the inputs put 0, 1, h-1, h, h+1 and q-1 into the last limb's coefficient form at the ends of the limb and on both sides
of the first column-tile boundary."""
import ctypes as C

import numpy as np
import pytest

from helpers import rescale_round as RR
from helpers import rescale_round_sizes as RS
from helpers import rlwe

pytestmark = pytest.mark.gpu
U = np.uint64
FHE_ERR_INVALID, FHE_ERR_UNSUPPORTED = 1, 3
SENTINEL = 0xA5A5A5A5A5A5A5A5

PRIME_SETS = RR.PRIME_SETS


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


_moduli, _same = RR.moduli, RR.same


# ------------------------------------------------------------------------------------------------ fhe_rescale, every route
@pytest.mark.parametrize("kind", list(PRIME_SETS))
@pytest.mark.parametrize("logn", [4, 8, 12, 13])
def test_rescale_nearest_on_every_route(F, eng, logn, kind):
    from oracle.keyswitch_ref import rescale_ref
    L, K = 3, 1
    qs = _moduli(F, logn, kind, K)
    t = eng.tables(logn, qs)
    ks = F.KeySwitch(eng, t, L, K, 1)
    assert ks.rescale_rounding is False
    q, h = qs[L - 1], (qs[L - 1] - 1) // 2
    cases = [(n, RR.dictated_parts(qs, L, logn, n, seed=100 * logn + n)) for n in (1, 2, 3)]
    cases.append((2, RR.dictated_parts(qs, L, logn, 2, seed=1, fill=h)))
    cases.append((3, RR.dictated_parts(qs, L, logn, 3, seed=2, fill=h + 1)))
    rng = np.random.default_rng(logn)
    cases.append((2, np.stack([np.stack([rng.integers(0, qj, 1 << logn, dtype=U) for qj in qs[:L]]) for _ in range(2)])))
    ks.set_rescale_rounding(True)
    assert ks.rescale_rounding is True
    for i, (n, parts) in enumerate(cases):
        _same(ks.rescale(eng.upload(parts), n), RR.round_rescale_ref(parts, qs, L, logn, True), f"nearest, case {i}, {n} parts")
    # the setter leaves nothing behind: mode 0 on the same plan gives the flooring words again
    ks.set_rescale_rounding(False)
    assert ks.rescale_rounding is False
    for n, parts in (cases[1], cases[3]):
        _same(ks.rescale(eng.upload(parts), n), rescale_ref(parts, qs, L, logn), f"floor after nearest, {n} parts")


# ------------------------------------------------------------------------------------------------ fhe_hmult, both routes
_hmult_case, _hmult_want = RR.hmult_case, RR.hmult_want


@pytest.mark.parametrize("kind", list(PRIME_SETS))
@pytest.mark.parametrize("logn,K,dnum,fusable", [(13, 2, 2, True), (12, 1, 1, False)])
def test_hmult_nearest_on_both_routes(F, eng, logn, K, dnum, fusable, kind):
    L = 3
    qs, a0, a1, b0, b1, key = _hmult_case(F, logn, kind, L, K, dnum, seed=7 * logn + K)
    t = eng.tables(logn, qs)
    ks = F.KeySwitch(eng, t, L, K, dnum)
    up = [eng.upload(x) for x in (a0, a1, b0, b1, key)]
    w0, w1 = _hmult_want(qs, a0, a1, b0, b1, key, L, K, dnum, logn, True)
    ks.set_rescale_rounding(True)
    try:
        for fused in ((1, 0) if fusable else (1,)):
            eng.set_option("hmult_fused_rescale", fused)
            o0, o1 = ks.hmult(*up, rescale=True)
            _same(o0, w0, f"part 0, hmult_fused_rescale = {fused}")
            _same(o1, w1, f"part 1, hmult_fused_rescale = {fused}")
    finally:
        eng.set_option("hmult_fused_rescale", 1)
    ks.set_rescale_rounding(False)
    f0, f1 = _hmult_want(qs, a0, a1, b0, b1, key, L, K, dnum, logn, False)
    o0, o1 = ks.hmult(*up, rescale=True)
    _same(o0, f0, "floor after nearest, part 0")
    _same(o1, f1, "floor after nearest, part 1")


def test_fused_route_is_the_one_taken_and_its_y_is_dictated(F, eng):
    """logn 13, K 2: a sharded plan of world 1 over the same shape says the multiply is fusable; and the fused route on a relinearised
    product whose last limb is dictated: the key is zero, so the key switch adds nothing and v = (d0, d1) -- the rescale's y is the
    coefficient form of d0's and d1's last limbs, built here from the branch words (b = (1, 0): d0 = a0, d1 = a1)"""
    from fhe_reliability_gpu_amd.dist import ShardedKeySwitch
    logn, L, K, dnum = 13, 3, 2, 2
    N = 1 << logn
    qs = _moduli(F, logn, "50+61last", K)
    t = eng.tables(logn, qs)
    sh = ShardedKeySwitch(eng, t, L, K, dnum)
    assert sh.fused_rescale
    parts = RR.dictated_parts(qs, L, logn, 2, seed=77)
    one = np.ones((L, N), dtype=U)          # the NTT form of the constant 1
    zero = np.zeros((L, N), dtype=U)
    key = np.zeros((dnum, 2, L + K, N), dtype=U)
    ks = F.KeySwitch(eng, t, L, K, dnum)
    ks.set_rescale_rounding(True)
    want = RR.round_rescale_ref(parts, qs, L, logn, True)
    assert (want != RR.round_rescale_ref(parts, qs, L, logn, False)).any()
    try:
        for fused in (1, 0):
            eng.set_option("hmult_fused_rescale", fused)
            o0, o1 = ks.hmult(eng.upload(parts[0]), eng.upload(parts[1]), eng.upload(one), eng.upload(zero), eng.upload(key), rescale=True)
            _same(o0, want[0], f"part 0, fused = {fused}")
            _same(o1, want[1], f"part 1, fused = {fused}")
    finally:
        eng.set_option("hmult_fused_rescale", 1)


# ------------------------------------------------------------------------------------------------ refusals
def test_plain_modulus_and_rounding_exclude_each_other(F, eng):
    from fhe_reliability_gpu_amd._lib import lib
    logn, L, K = 8, 3, 1
    qs = _moduli(F, logn, "50", K)
    ks = F.KeySwitch(eng, eng.tables(logn, qs), L, K, 1)
    ks.set_plain_modulus(65537)
    assert lib.fhe_keyswitch_set_rescale_rounding(ks._h, 1) == FHE_ERR_UNSUPPORTED
    assert b"plain modulus" in lib.fhe_last_error()
    assert ks.rescale_rounding is False
    ks.set_plain_modulus(0)
    ks.set_rescale_rounding(True)
    assert lib.fhe_keyswitch_set_plain_modulus(ks._h, 65537) == FHE_ERR_UNSUPPORTED
    assert b"nearest" in lib.fhe_last_error()
    # the plan still rounds, and still rescales
    parts = RR.dictated_parts(qs, L, logn, 2, seed=3)
    _same(ks.rescale(eng.upload(parts), 2), RR.round_rescale_ref(parts, qs, L, logn, True), "after the refused plain modulus")
    assert lib.fhe_keyswitch_set_rescale_rounding(ks._h, 2) == FHE_ERR_INVALID
    assert ks.rescale_rounding is True
    # L = 1: the setter accepts, the rescale refuses as it always did
    k1 = F.KeySwitch(eng, eng.tables(logn, qs[:2]), 1, 1, 1)
    k1.set_rescale_rounding(True)
    assert k1.rescale_rounding is True


@pytest.fixture(scope="module")
def refusal_case(F, eng):
    logn, L, K, dnum = 13, 3, 2, 2
    qs, a0, a1, b0, b1, key = _hmult_case(F, logn, "50", L, K, dnum, seed=11)
    t = eng.tables(logn, qs)
    ks = F.KeySwitch(eng, t, L, K, dnum)
    return dict(logn=logn, L=L, K=K, dnum=dnum, qs=qs, t=t, ks=ks, ab=F.Abft(eng, t), host=(a0, a1, b0, b1, key),
                dev=[eng.upload(x) for x in (a0, a1, b0, b1, key)])


def _sentinel(eng, words):
    return eng.upload(np.full(words, SENTINEL, dtype=U))


def _untouched(buf, what):
    assert (buf.download() == U(SENTINEL)).all(), f"{what} was written by a refused call"


CALLS = ["rescale_checked", "rescale_sealed", "hmult_checked", "hmult_sealed", "hmult_sealed_fused", "hmult_sealed_fused_key", "hmult_sealed_out",
         "hmult_sealed_repair"]


@pytest.mark.parametrize("call", CALLS)
def test_checked_and_sealed_rescaling_calls_refuse_a_rounding_plan(F, eng, refusal_case, call):
    """status FHE_ERR_UNSUPPORTED, outputs and flags at their sentinel, and the rescale hook the call owns is gone: a checked rescale
    in mode 0 right after it runs clean"""
    from fhe_reliability_gpu_amd._lib import check, lib
    from oracle.keyswitch_ref import rescale_ref
    c = refusal_case
    ks, ab, L, N = c["ks"], c["ab"], c["L"], 1 << c["logn"]
    a0, a1, b0, b1, key = c["dev"]
    out0, out1, flags = _sentinel(eng, 3 * (L - 1) * N), _sentinel(eng, (L - 1) * N), _sentinel(eng, 1 << 14)
    parts = np.stack([c["host"][0], c["host"][1]])
    d_in = eng.upload(parts)
    seal_a, seal_b = _sentinel(eng, 2 * 2 * L), _sentinel(eng, 2 * 2 * L)
    null4 = (C.c_void_p * 4)()
    null2 = (C.c_void_p * 2)()
    ks.set_rescale_rounding(True)
    try:
        check(lib.fhe_ctx_inject_fault_rescale(eng._h, 3, 0, 0, 5, 30))
        e, p, A = eng._h, ks._h, ab._h
        hm = (e, p, out0.ptr, out1.ptr, a0.ptr, a1.ptr, b0.ptr, b1.ptr, key.ptr, 1, A)
        if call == "rescale_checked":
            rc = lib.fhe_rescale_checked(e, p, out0.ptr, d_in.ptr, 2, A, flags.ptr, None)
        elif call == "rescale_sealed":
            rc = lib.fhe_rescale_sealed(e, p, out0.ptr, d_in.ptr, 2, A, seal_a.ptr, seal_b.ptr, flags.ptr, None)
        elif call == "hmult_checked":
            rc = lib.fhe_hmult_checked(*hm, flags.ptr, None)
        elif call == "hmult_sealed_repair":
            rc = lib.fhe_hmult_sealed_repair(*hm, null4, null4, None, None, null2, null2, flags.ptr, None)
        else:
            rc = getattr(lib, "fhe_" + call)(*hm, null4, None, null2, flags.ptr, None)
        assert rc == FHE_ERR_UNSUPPORTED, (call, rc, lib.fhe_last_error())
        assert b"nearest" in lib.fhe_last_error()
        eng.sync()
        for buf, what in ((out0, "out0"), (out1, "out1"), (flags, "flags"), (seal_b, "seal_out")):
            _untouched(buf, f"{call}: {what}")
    finally:
        ks.set_rescale_rounding(False)
    # the armed hook went with the refused call
    o, fl = ks.rescale_checked(d_in, ab, 2)
    for name, f in fl.items():
        assert not np.asarray(f).any(), f"{call}: the rescale hook survived the refusal and hit stage {name}"
    _same(o, rescale_ref(parts, c["qs"], L, c["logn"]), f"{call}: the checked rescale after the refusal")


def test_checked_multiply_without_rescale_runs_on_a_rounding_plan(F, eng, refusal_case):
    c = refusal_case
    ks, ab = c["ks"], c["ab"]
    ks.set_rescale_rounding(True)
    try:
        w0, w1 = ks.hmult(*c["dev"], rescale=False)
        o0, o1, fl = ks.hmult_checked(*c["dev"], ab, rescale=False)
        _same(o0, w0.download(), "part 0")
        _same(o1, w1.download(), "part 1")
        assert not np.asarray(fl["tensor"]).any()
        for name, f in fl["keyswitch"].items():
            assert not np.asarray(f).any(), name
    finally:
        ks.set_rescale_rounding(False)


# ------------------------------------------------------------------------------------------------ sharded phases
def test_one_rank_phase_path_equals_the_single_call(F, eng):
    RS.one_rank_phase_path(F, eng, 13, [50] * 7, L=5, K=2, dnum=3)


def test_two_ranks_in_one_process(F, eng):
    """both ranks' plans in one process, the host doing the collectives: fhe_rescale_shard_* and the fused multiply's finish, gathered
    limbs against the single-device words (which test_hmult_nearest_on_both_routes holds against the helper)"""
    RS.two_ranks_in_one_process(F, eng, 13, [50] * 6, L=4, K=2, dnum=2)


# ------------------------------------------------------------------------------------------------ decryption level
def test_rescaled_ciphertext_decrypts_to_the_rounded_value(F, eng):
    """CKKS form, N = 2^12, L = 3: the input decrypts to v exactly (decrypt of the very parts that are rescaled), so the input noise
    term is zero.  Two assertions, both derived in helpers/rescale_round.py from |r_i| <= h per part:
    * |q dec' - v| <= h (1 + |s|_1): the bound the feature is specified by, "within 1/2 (1 + |s|_1)" of v / q, stated exactly in
      integers (h / q < 1/2);
    * |dec' - div_round(v, q)| < 1/2 (1 + 1 + |s|_1): against the ROUNDED value the comparison value's own rounding adds its 1/2;
      strict, because (h / q) (2 + |s|_1) < 1/2 (2 + |s|_1); compared doubled."""
    logn, L, K, dnum = 12, 3, 1, 1
    N = 1 << logn
    qs = F.create_moduli(N, [50] * (L + K))
    party = rlwe.Party(N, qs, L, K, dnum, t=0, seed=12)
    q = qs[L - 1]
    m = [party.rnd.randrange(-(1 << 70), 1 << 70) for _ in range(N)]
    c0, c1 = party.encrypt(m)
    v = party.decrypt([c0, c1])
    ks = F.KeySwitch(eng, eng.tables(logn, qs), L, K, dnum)
    ks.set_rescale_rounding(True)
    out = ks.rescale(eng.upload(np.stack([c0, c1])), 2).download().reshape(2, L - 1, N)
    dec = party.decrypt([out[0], out[1]], limbs=L - 1)
    bound2 = RR.nearest_bound_2x(party.s, 2)
    worst2 = max(abs(2 * (d - rlwe.div_round(x, q))) for d, x in zip(dec, v))
    print(f"nearest: 2 |dec' - round(v / q)| reaches {worst2}, bound {bound2}")
    assert worst2 < bound2
    h = (q - 1) // 2
    assert max(abs(q * d - x) for d, x in zip(dec, v)) <= h * (bound2 - 1)
