"""The reference of the round-to-nearest rescale (tests/helpers/rescale_round.py) against itself and the existing oracle: its two
independent statements agree, its flooring mode is oracle.keyswitch_ref.rescale_ref word for word, nearest minus floor is the
indicator of [C]_q > h, and only the nearest words meet the rounding definition |centred(q c' - C mod Q)| <= h."""
import numpy as np
import pytest

from helpers import rescale_round as RR
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
