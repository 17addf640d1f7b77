"""The round-to-nearest rescale at every two-launch size and limb layout.  tests/test_gpu_rescale_round.py runs the column passes that
round -- k_ntt_col_round (fhe_rescale) and k_ntt_col_addsrc<.., true> (fused fhe_hmult) -- at 2^13 only, always with L = 3, and never
with an option that sends N >= 2^13 through k_round_residues.  Here:
  a. fhe_rescale at 2^14 .. 2^17 on both arithmetic paths, and with a last limb of the other path than the limbs it is reduced to;
  b. fhe_rescale with L = 5 and the paths alternating: four runs in rescale_finish, off = 0 .. 3;
  c. the fused fhe_hmult at 2^14 .. 2^17, and with several runs in ks_finish_rescale_end;
  d. ntt_resident and ntt_mode 1, whose rescale forms the rounded residues in a launch of their own at N >= 2^13;
  e. the sharded phases at 2^15 with the alternating layout, the second rank's slab starting at clo > 0.
After the nearest words every test sets mode 0 on the same plan and asks for the flooring oracle's words, so a dispatch that ignored
the mode fails on one side or the other.  Every comparison is == against tests/helpers/rescale_round.py (nearest) and
oracle.keyswitch_ref (floor); the inputs put the branch words at the row and tile boundaries of each size's column matrix
(RR.ROW_LEN), and RR.references holds, for every case, that each 16-column tile of each output limb tells nearest from floor.  Shapes,
case builders and the sharded bodies: tests/helpers/rescale_round_sizes.py."""
import numpy as np
import pytest

from helpers import rescale_round as RR
from helpers import rescale_round_sizes as RS

pytestmark = pytest.mark.gpu
U = np.uint64


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


def _rescale_both_modes(eng, ks, qs, L, logn, cases, floor_again, what):
    """nearest on every case, then mode 0 on the same plan on the cases named in floor_again"""
    refs = {name: RR.references(parts, qs, L, logn, differs, f"{what}: {name}") for name, parts, differs in cases}
    dev = {name: eng.upload(parts) for name, parts, _ in cases}
    ks.set_rescale_rounding(True)
    for name, parts, _ in cases:
        RR.same(ks.rescale(dev[name], len(parts)), refs[name][0], f"{what}: nearest, {name}")
    ks.set_rescale_rounding(False)
    for name, parts, _ in cases:
        if name in floor_again:
            RR.same(ks.rescale(dev[name], len(parts)), refs[name][1], f"{what}: floor after nearest, {name}")


# ------------------------------------------------------------------------------------------------ a. fhe_rescale, every size x both paths
@pytest.mark.parametrize("logn,kind", RS.SIZES_RESCALE)
def test_rescale_nearest_at_every_two_launch_size(F, eng, logn, kind):
    L, K = 3, 1
    qs = RR.moduli(F, logn, kind, K)
    ks = F.KeySwitch(eng, eng.tables(logn, qs), L, K, 1)
    cases = RS.rescale_cases(qs, L, logn, RS.case_seed(logn, kind))
    assert [len(p) for _, p, _ in cases] == [1, 2, 3, 1, 1, 2]
    _rescale_both_modes(eng, ks, qs, L, logn, cases, ("dictated, 2 parts", "random, 2 parts"), f"2^{logn} {kind}")


# ------------------------------------------------------------------------------------------------ b. more than one run
@pytest.mark.parametrize("logn,kind", RS.SIZES_RUNS)
def test_rescale_nearest_over_four_runs(F, eng, logn, kind):
    L, K = 5, 2
    qs = RR.moduli(F, logn, kind, K)
    t = eng.tables(logn, qs)
    assert [t.paths[j] != t.paths[j + 1] for j in range(L - 2)] == [True] * (L - 2)      # every remaining limb is a run of its own
    ks = F.KeySwitch(eng, t, L, K, 1)
    _rescale_both_modes(eng, ks, qs, L, logn, RS.runs_cases(qs, L, logn, RS.case_seed(logn, kind)), ("random, 2 parts",), f"2^{logn} {kind}")


# ------------------------------------------------------------------------------------------------ c. fused fhe_hmult
def _hmult_both_routes(eng, ks, up, want, what, routes=(1, 0)):
    try:
        for fused in routes:
            eng.set_option("hmult_fused_rescale", fused)
            o0, o1 = ks.hmult(*up, rescale=True)
            RR.same(o0, want[0], f"{what}, part 0, hmult_fused_rescale = {fused}")
            RR.same(o1, want[1], f"{what}, part 1, hmult_fused_rescale = {fused}")
    finally:
        eng.set_option("hmult_fused_rescale", 1)


@pytest.mark.parametrize("logn,kind,L", RS.SIZES_HMULT)
def test_fused_hmult_nearest_at_every_two_launch_size(F, eng, logn, kind, L):
    from fhe_reliability_gpu_amd.dist import ShardedKeySwitch
    K = dnum = 2
    N = 1 << logn
    qs, a0, a1, b0, b1, key = RR.hmult_case(F, logn, kind, L, K, dnum, seed=RS.case_seed(logn, kind))
    t = eng.tables(logn, qs)
    assert ShardedKeySwitch(eng, t, L, K, dnum).fused_rescale          # a plan of world 1 over the same shape: the fused route is taken
    ks = F.KeySwitch(eng, t, L, K, dnum)
    what = f"2^{logn} {kind}"
    # y dictated: zero key, b = (1, 0), so the relinearised product is (a0, a1) and y the coefficient form of their last limbs
    parts = RS.dictated_hmult_parts(qs, L, logn)
    dict_near, _ = RR.references(parts, qs, L, logn, True, f"{what}: dictated y")
    one, zero = np.ones((L, N), dtype=U), np.zeros((L, N), dtype=U)          # the NTT form of the constants 1 and 0
    dict_up = [eng.upload(x) for x in (parts[0], parts[1], one, zero, np.zeros((dnum, 2, L + K, N), dtype=U))]
    # random key
    near, floor = RR.references(RR.hmult_relin_ref(qs, a0, a1, b0, b1, key, L, K, dnum, logn), qs, L, logn, True, f"{what}: random key")
    up = [eng.upload(x) for x in (a0, a1, b0, b1, key)]
    ks.set_rescale_rounding(True)
    _hmult_both_routes(eng, ks, dict_up, dict_near, f"{what}: dictated y")
    _hmult_both_routes(eng, ks, up, near, f"{what}: random key")
    ks.set_rescale_rounding(False)
    _hmult_both_routes(eng, ks, up, floor, f"{what}: floor after nearest", routes=(1,))


# ------------------------------------------------------------------------------------------------ d. the plain route at N >= 2^13
@pytest.mark.parametrize("kind", RS.PLAIN_KINDS)
@pytest.mark.parametrize("logn,option", RS.SIZES_PLAIN)
def test_rounded_residues_in_their_own_launch_at_two_launch_sizes(F, eng, logn, option, kind):
    """ntt_resident / ntt_mode 1: rescale_finish takes the route of the single-launch sizes -- k_round_residues, the plain transform,
    k_sub_scale -- and a multiply with K = 2, fused by default, relinearises and then rescales through it"""
    from fhe_reliability_gpu_amd.dist import ShardedKeySwitch
    L, K, dnum = 3, 2, 2
    qs, a0, a1, b0, b1, key = RS.plain_hmult_case(F, logn, kind)
    t = eng.tables(logn, qs)
    ks = F.KeySwitch(eng, t, L, K, dnum)
    sh = ShardedKeySwitch(eng, t, L, K, dnum)
    what = f"2^{logn} {kind}, {option} = 1"
    near, floor = RR.references(RR.hmult_relin_ref(qs, a0, a1, b0, b1, key, L, K, dnum, logn), qs, L, logn, True, f"{what}: multiply")
    up = [eng.upload(x) for x in (a0, a1, b0, b1, key)]
    assert sh.fused_rescale
    eng.set_option(option, 1)
    try:
        assert not sh.fused_rescale
        _rescale_both_modes(eng, ks, qs, L, logn, RS.plain_cases(qs, L, logn, RS.case_seed(logn, kind)), ("dictated, 2 parts", "random, 2 parts"), what)
        ks.set_rescale_rounding(True)
        _hmult_both_routes(eng, ks, up, near, f"{what}: multiply, nearest", routes=(1,))
        ks.set_rescale_rounding(False)
        _hmult_both_routes(eng, ks, up, floor, f"{what}: multiply, floor after nearest", routes=(1,))
        eng.check()
    finally:
        eng.set_option(option, 0)


# ------------------------------------------------------------------------------------------------ e. sharded phases at a second size
SHARD = dict(RS.SHARD, row_len=RR.ROW_LEN[RS.SHARD["logn"]], floor_again=True)


def test_one_rank_phase_path_at_2_15_over_alternating_limbs(F, eng):
    RS.one_rank_phase_path(F, eng, **SHARD)


def test_two_ranks_at_2_15_the_second_slab_starts_on_the_other_path(F, eng):
    """the rescale phases and the fused finish against the reference, nearest and then mode 0 on the same two plans"""
    lays = RS.two_ranks_in_one_process(F, eng, **SHARD)
    clo, paths = lays[1]["clo"], eng.tables(15, F.create_moduli(1 << 15, SHARD["bits"])).paths
    assert 0 < clo < SHARD["L"] - 1 and paths[clo] != paths[0]
