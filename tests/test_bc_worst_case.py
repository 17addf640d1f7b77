"""The adversarial input builder of the base-conversion edge tests (tests/helpers/bc_worst_case.py), checked on the CPU: the digits
it dictates are the digits an independent mixed-radix decomposition recovers, its expected words agree with the C oracle, and the
all-maximal column really reaches the regime the FP64 kernels' exactness bound speaks of (eight terms of S2 summing past 2^51)."""
import random

import numpy as np
import pytest

from oracle import cport as O
from helpers import bc_worst_case as W

N = 1 << 10
K = 3
SIZES = [1, 2, 8, 9, 16]


def _plan(bits, m, k=K):
    qs = O.gen_primes(N, bits, m + k)
    return qs[:m], qs[m:]


def test_split_is_round_to_nearest_even():
    for v, want in ((0, (0, 0)), (W.TIE - 1, (0, W.TIE - 1)), (W.TIE, (0, W.TIE)), (W.TIE + 1, (1, -W.TIE + 1)),
                    (W.HALF + W.TIE, (2, -W.TIE)), (2 * W.HALF + W.TIE, (2, W.TIE)), (3 * W.HALF + W.TIE, (4, -W.TIE)),
                    ((1 << 50) - 1, (1 << 25, -1))):
        assert W.split(v) == want
        # the same through the arithmetic the kernels use: rint, then a fused multiply-add (exact here: both are below 2^53)
        hi = float(np.rint(np.float64(v) * 2.0 ** -25))
        assert (int(hi), v - int(hi) * W.HALF) == want


@pytest.mark.parametrize("bits", [50, 61])
@pytest.mark.parametrize("m", SIZES)
def test_chosen_digits_are_the_digits_recovered(bits, m):
    mi, mo = _plan(bits, m)
    cols = W.worst_columns(mi, mo)
    names = [n for n, _ in cols]
    assert len(set(names)) == len(names)
    assert {"zero", "max", "tie-even", "tie-odd", "alternate0", "alternate1"} <= set(names)
    assert all(f"{t}[{o}]" in names for t in ("S1+", "S1-", "S0") for o in range(len(mo)))
    assert all(f"single[{l}]" in names for l in range(m))
    rnd = random.Random(m * 100 + bits)
    cols += [(f"random{i}", [rnd.randrange(p) for p in mi]) for i in range(64)]
    for name, digs in cols:
        r = W.residues_from_digits(mi, digs)
        got, words = W.exact_reference(mi, mo, r)
        assert got == digs, name
        x = sum(c * w for c, w in zip(digs, W._prefix_products(mi)))
        assert words == [x % q for q in mo], name


@pytest.mark.parametrize("m", SIZES)
def test_columns_hit_what_their_names_say(m):
    mi, mo = _plan(50, m)
    cols = dict(W.worst_columns(mi, mo))
    assert cols["zero"] == [0] * m and cols["max"] == [p - 1 for p in mi]
    for l in range(m):
        assert W.split(cols["tie-even"][l])[1] == W.TIE and W.split(cols["tie-odd"][l])[1] == -W.TIE
        assert W.split(cols["tie-even"][l])[0] >= W.split(mi[l] - 1)[0] - 2      # next to the top of the range
    rnd = random.Random(m)
    for o, q in enumerate(mo):
        ks = W.split_constants(mi, q)
        for E, e1, e0 in ks:
            assert E == e1 * W.HALF + e0 and abs(e0) <= W.TIE and 0 <= e1 <= W.HALF
        for sign, tag in ((1, "+"), (-1, "-")):
            digs = cols[f"S1{tag}[{o}]"]
            for l, ((_, e1, e0), c) in enumerate(zip(ks, digs)):
                c1, c0 = W.split(c)
                term = sign * (c1 * e0 + c0 * e1)
                # the term is on the wanted side (or p leaves no digit there), and no random digit does better
                assert term >= 0 or l == 0
                assert all(term >= sign * (a * e0 + b * e1) for a, b in (W.split(rnd.randrange(mi[l])) for _ in range(64)))
        for (_, _, e0), c in zip(ks, cols[f"S0[{o}]"]):
            c0 = W.split(c)[1]
            assert c0 * e0 >= (W.TIE - 1) * abs(e0)
        # and the sums they were built for beat the all-maximal column's
        s_max = W.split_sums(mi, q, cols["max"])
        assert W.split_sums(mi, q, cols[f"S1+[{o}]"])[1] >= s_max[1] >= W.split_sums(mi, q, cols[f"S1-[{o}]"])[1]
        assert W.split_sums(mi, q, cols[f"S0[{o}]"])[2] >= s_max[2]


@pytest.mark.parametrize("bits", [50, 61])
@pytest.mark.parametrize("m", SIZES)
def test_oracle_agrees_with_the_integer_reference(bits, m):
    mi, mo = _plan(bits, m)
    names, res, want = W.worst_residues(mi, mo)
    rnd = random.Random(m * 1000 + bits)
    for i in range(64):
        r = [rnd.randrange(p) for p in mi]
        names.append(f"random{i}")
        res.append(r)
        want.append(W.exact_reference(mi, mo, r)[1])
    x = np.array(res, dtype=np.uint64).T                       # [m][columns]
    got = O.baseconv_exact(np.ascontiguousarray(x), mi, mo)     # [k][columns]
    bad = [names[i] for i in np.nonzero((got.T != np.array(want, dtype=np.uint64)).any(axis=1))[0]]
    assert not bad, bad


@pytest.mark.parametrize("m", [8, 9, 16])
def test_maximal_column_reaches_the_exactness_regime(m):
    """Eight products c1 e1 of at most 2^50 each: the bound of the kernels' comment is 2^53.  Random digits sit a factor 2 to 4 below
    it; the all-maximal column must put the first eight terms of S2 past 2^51 for some output, and the S1 columns past 2^50."""
    pool = O.gen_primes(N, 50, m + 32)
    mi, outs = pool[:m], pool[m:]
    top = [p - 1 for p in mi]
    s2 = [W.split_sums(mi, q, top, 8)[0] for q in outs[:K]]
    if max(s2) < 1 << 51:                                       # not with the first outputs: a larger pool
        s2 = [W.split_sums(mi, q, top, 8)[0] for q in outs]
    print(f"m = {m}: largest S2 over eight terms = {max(s2)} = 2^{np.log2(float(max(s2))):.3f}")
    assert 1 << 51 <= max(s2) <= 1 << 53
    cols = dict(W.worst_columns(mi, outs[:K]))
    s1 = [abs(W.split_sums(mi, q, cols[f"S1{tag}[{o}]"], 8)[1]) for o, q in enumerate(outs[:K]) for tag in "+-"]
    print(f"m = {m}: largest |S1| over eight terms = {max(s1)} = 2^{np.log2(float(max(s1))):.3f}")
    assert 1 << 50 <= max(s1) <= 1 << 53
