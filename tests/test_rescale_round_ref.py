"""The reference of the round-to-nearest rescale (tests/helpers/rescale_round.py) against itself and the existing oracle: its two
independent statements agree, its flooring mode is oracle.keyswitch_ref.rescale_ref word for word, nearest minus floor is the
indicator of [C]_q > h, and only the nearest words meet the rounding definition |centred(q c' - C mod Q)| <= h."""
import numpy as np
import pytest

from helpers import rescale_round as RR
from helpers import rescale_round_sizes as RS
from helpers import rlwe
from oracle import cport as O
from oracle.keyswitch_ref import rescale_ref

U = np.uint64
CASES = [(4, [50, 50, 50]), (6, [61, 61, 61]), (6, [50, 50, 61]), (6, [61, 61, 50]), (6, [30, 30, 61]), (8, [50, 61, 30, 50])]


def _moduli(logn, bits):
    N, out = 1 << logn, []
    for b in sorted(set(bits)):
        ps = O.gen_primes(N, b, bits.count(b))
        out.append((b, list(ps)))
    pool = dict(out)
    return [pool[b].pop() for b in bits]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"2^{c[0]}-" + "/".join(map(str, c[1])))
def case(request):
    logn, bits = request.param
    qs = _moduli(logn, bits)
    L = len(qs)
    parts = np.concatenate([RR.dictated_parts(qs, L, logn, 3, seed=logn), RR.dictated_parts(qs, L, logn, 1, seed=1, fill=(qs[-1] - 1) // 2),
                            RR.dictated_parts(qs, L, logn, 1, seed=2, fill=(qs[-1] + 1) // 2)])
    return logn, qs, L, parts


def test_the_two_statements_agree(case):
    logn, qs, L, parts = case
    for nearest in (True, False):
        a = RR.round_rescale_ref(parts, qs, L, logn, nearest)
        b = RR.round_rescale_int(parts, qs, L, logn, nearest)
        assert a.shape == b.shape == (len(parts), L - 1, 1 << logn)
        assert (a == b).all(), nearest


def test_flooring_mode_is_the_oracles_rescale(case):
    logn, qs, L, parts = case
    assert (RR.round_rescale_ref(parts, qs, L, logn, False) == rescale_ref(parts, qs, L, logn)).all()


def test_nearest_minus_floor_is_the_indicator_of_the_upper_half(case):
    logn, qs, L, parts = case
    q = qs[L - 1]
    h = (q - 1) // 2
    seen = set()
    for part in parts:
        Cs = RR.lift(part, qs, logn)
        near, floor = RR.rescaled_ints(Cs, q, True), RR.rescaled_ints(Cs, q, False)
        for c, n, f in zip(Cs, near, floor):
            up = c % q > h
            assert n - f == (1 if up else 0)
            seen.add(up)
    assert seen == {True, False}


def test_only_the_nearest_words_meet_the_rounding_definition(case):
    logn, qs, L, parts = case
    q, Q = qs[L - 1], rlwe.prod(qs)
    h = (q - 1) // 2
    near = RR.round_rescale_ref(parts, qs, L, logn, True)
    for part, out in zip(parts, near):
        Cs, cs = RR.lift(part, qs, logn), RR.lift(out, qs[:L - 1], logn)
        assert all(abs(rlwe.centred(q * c2 - c, Q)) <= h for c, c2 in zip(Cs, cs))
    # a last limb whose remainders are all q - 1: the flooring words miss the definition at every coefficient
    worst = RR.dictated_parts(qs, L, logn, 1, seed=5, fill=q - 1)
    floor = rescale_ref(worst, qs, L, logn)
    Cs, cs = RR.lift(worst[0], qs, logn), RR.lift(floor[0], qs[:L - 1], logn)
    assert all(rlwe.centred(q * c2 - c, Q) == -(q - 1) for c, c2 in zip(Cs, cs))
    assert q - 1 > h
    cs = RR.lift(RR.round_rescale_ref(worst, qs, L, logn, True)[0], qs[:L - 1], logn)
    assert all(rlwe.centred(q * c2 - c, Q) == 1 for c, c2 in zip(Cs, cs))


def test_decryption_bound_is_twice_as_tight_as_the_floors_worst_case():
    """the helper's bound, from |r| <= h: 1 + sum |s^i|_1 (doubled); s = 1 + X: |s|_1 = 2, |s^2|_1 = 4"""
    s = [1, 1] + [0] * 14
    assert RR.l1_powers(s, 3) == [1, 2, 4]
    assert RR.nearest_bound_2x(s, 2) == 4 and RR.nearest_bound_2x(s, 3) == 8


# ------------------------------------------------------------------------------------------------ the two-launch sizes' positions
@pytest.mark.parametrize("logn", sorted(RR.ROW_LEN))
def test_row_positions_are_inside_the_limb_and_distinct(logn):
    N, row_len = 1 << logn, RR.ROW_LEN[logn]
    base, pos = RR.branch_positions(N), RR.branch_positions(N, row_len=row_len)
    assert pos[:len(base)] == base and len(pos) == len(base) + 6
    assert all(0 <= p < N for p in pos) and len(set(pos)) == len(pos)
    row, tile = lambda p: p // row_len, lambda p: p % row_len // RR.TILE_COLS
    assert {row(p) for p in pos} == {0, 1, N // row_len - 1}
    assert (row(row_len), tile(row_len)) == (1, 0) and (tile(row_len + 15), tile(row_len + 16)) == (0, 1)
    assert (row(N - row_len), tile(N - row_len)) == (N // row_len - 1, 0)
    assert (tile(N - 17), tile(N - 16), tile(N - 1)) == (row_len // 16 - 2, row_len // 16 - 1, row_len // 16 - 1)
    classes = RR.position_classes(N, row_len)
    assert set().union(*classes.values()) == set(pos)


@pytest.mark.parametrize("logn", sorted(RR.ROW_LEN))
def test_every_branch_word_reaches_every_position_class_over_three_parts(logn):
    """on the y the parts are built from; a given row_len leaves the earlier positions' words, and the default argument the whole y, as
    they were"""
    N, row_len, q = 1 << logn, RR.ROW_LEN[logn], O.gen_primes(1 << logn, 50, 1)[0]
    words = RR.branch_words(q)
    ys = [RR.dictated_y(q, logn, p, np.random.default_rng(p), row_len) for p in range(3)]
    for name, at in RR.position_classes(N, row_len).items():
        assert {int(y[a]) for y in ys for a in at} == set(words), name
    for p, y in enumerate(ys):
        old = RR.dictated_y(q, logn, p, np.random.default_rng(p))
        new_pos = RR.branch_positions(N, row_len=row_len)[len(RR.branch_positions(N)):]
        keep = np.ones(N, dtype=bool)
        keep[new_pos] = False
        assert (y[keep] == old[keep]).all()
        assert [int(old[a]) for a in RR.branch_positions(N)] == [words[(p + k) % 6] for k in range(5)]


# ------------------------------------------------------------------------------------------------ more than one run of remaining limbs
@pytest.mark.parametrize("kind", list(RR.ALTERNATING))
@pytest.mark.parametrize("n_parts", [1, 2, 3])
def test_the_two_statements_agree_where_the_remaining_limbs_alternate_paths(kind, n_parts):
    logn, L = 6, 5
    qs = _moduli(logn, RR.limb_bits(kind, 0))
    h = (qs[-1] - 1) // 2
    parts = np.concatenate([RR.dictated_parts(qs, L, logn, n_parts, seed=n_parts), RR.dictated_parts(qs, L, logn, 1, seed=1, fill=h),
                            RR.dictated_parts(qs, L, logn, 1, seed=2, fill=h + 1), RR.random_parts(qs, L, logn, n_parts, seed=3)])
    for nearest in (True, False):
        a = RR.round_rescale_ref(parts, qs, L, logn, nearest)
        assert (a == RR.round_rescale_int(parts, qs, L, logn, nearest)).all(), nearest
    assert (RR.round_rescale_ref(parts, qs, L, logn, False) == rescale_ref(parts, qs, L, logn)).all()


# ------------------------------------------------------------------------------------------------ the GPU file's cases, on the CPU
@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


def test_the_tile_condition_fails_a_tile_that_floored():
    logn, L = 13, 3
    qs = _moduli(logn, [50, 50, 50])
    parts = RR.random_parts(qs, L, logn, 2, seed=0)
    near, floor = RR.references(parts, qs, L, logn)
    mixed = near.copy()
    mixed[1, 0, 48:64] = floor[1, 0, 48:64]
    with pytest.raises(AssertionError, match=r"1 of 2048 tiles, first \(part, limb, tile\) \[1, 0, 3\]"):
        RR.assert_every_tile_differs(mixed, floor)
    # y = h everywhere rounds nothing: the one case the condition is not asked of, and references() says so instead
    flat = RR.dictated_parts(qs, L, logn, 1, seed=0, fill=(qs[-1] - 1) // 2)
    with pytest.raises(AssertionError):
        RR.references(flat, qs, L, logn, differs=True)
    RR.references(flat, qs, L, logn, differs=False)


@pytest.mark.parametrize("logn", [13, 14])
def test_every_tile_of_every_gpu_case_tells_nearest_from_floor(F, logn):
    """every case tests/test_gpu_rescale_round_sizes.py builds at this size, from the same tables, functions and seeds.  2^15 .. 2^17: the
    GPU tests assert the same on the references they compute"""
    seen = 0
    for sizes, L, K, build in ((RS.SIZES_RESCALE, 3, 1, RS.rescale_cases), (RS.SIZES_RUNS, 5, 2, RS.runs_cases)):
        for ln, kind in sizes:
            if ln != logn:
                continue
            qs = RR.moduli(F, logn, kind, K)
            for name, parts, differs in build(qs, L, logn, RS.case_seed(logn, kind)):
                RR.references(parts, qs, L, logn, differs, f"2^{logn} {kind}: {name}")
                seen += 1
    for ln, option in RS.SIZES_PLAIN:
        for kind in RS.PLAIN_KINDS if ln == logn else ():
            qs, *ops = RS.plain_hmult_case(F, logn, kind)
            RR.references(RR.hmult_relin_ref(qs, *ops, 3, 2, 2, logn), qs, 3, logn, True, f"2^{logn} {kind}, {option}: multiply")
            for name, parts, differs in RS.plain_cases(qs, 3, logn, RS.case_seed(logn, kind)):
                RR.references(parts, qs, 3, logn, differs, f"2^{logn} {kind}, {option}: {name}")
                seen += 1
    for ln, kind, L in RS.SIZES_HMULT:
        if ln != logn:
            continue
        K = dnum = 2
        qs, *ops = RR.hmult_case(F, logn, kind, L, K, dnum, seed=RS.case_seed(logn, kind))
        RR.references(RR.hmult_relin_ref(qs, *ops, L, K, dnum, logn), qs, L, logn, True, f"2^{logn} {kind}: random key")
        RR.references(RS.dictated_hmult_parts(qs, L, logn), qs, L, logn, True, f"2^{logn} {kind}: dictated y")
        seen += 1
    assert seen


@pytest.mark.parametrize("shape", [dict(logn=13, bits=[50] * 7, L=5, K=2, dnum=3), dict(logn=13, bits=[50] * 6, L=4, K=2, dnum=2),
                                   dict(RS.SHARD, row_len=RR.ROW_LEN[RS.SHARD["logn"]])], ids=["2^13 L5", "2^13 L4", "2^15 alternating"])
def test_every_tile_of_the_sharded_cases_tells_nearest_from_floor(F, shape):
    """the inputs of the sharded bodies at the shapes the two GPU files call them with (the bodies assert the same on the GPU)"""
    logn, L, K, dnum, row_len = shape["logn"], shape["L"], shape["K"], shape["dnum"], shape.get("row_len")
    qs = F.create_moduli(1 << logn, shape["bits"])
    RR.references(RS.one_rank_parts(qs, L, logn, row_len), qs, L, logn, True, "one rank")
    ops, parts = RS.two_rank_inputs(qs, L, K, dnum, logn, row_len)
    RR.references(parts, qs, L, logn, True, "two ranks, rescale")
    RR.references(RR.hmult_relin_ref(qs, *ops, L, K, dnum, logn), qs, L, logn, True, "two ranks, multiply")
