"""The designed inputs of tests/helpers/harvey_cases.py held against the oracle, and the reason they exist shown on a model of
ArithU64 in Python integers: every comparison of the integer path is ``x >= 2q`` or ``x >= q``, random words never meet equality, the
families meet it thousands of times.  No GPU, no emulation, no library: the oracle and Python integers only.

What the mutants show (one ``>`` for one ``>=``; all of this is exact, there is no tolerance anywhere):

  canonical(), either line   wrong words on the families (q where the oracle has 0), no random vector notices
  forward fold               wrong words on one family only, fold_tail: an unfolded 2q is absorbed by the next fold or by canonical()
                             unless the LAST stage pairs it with an exact 0, which gives 4q -- one q more than canonical() removes
  inverse sum                NO input can show it in the output words: an unfolded sum 2q is a valid operand of every later step
                             (the difference X - Y + 2q stays below 2^64, the Shoup product takes any 64-bit word), and the last
                             stage's product puts every word back into [0, 2q).  What it breaks is the documented range [0, 2q)
                             of the inverse's operands, and that is what catches it here and in the emulation's range assertions.
  barrett128, either fix-up  NO input can show it: the two fix-ups are the same comparison, and the quotient estimate is never more
                             than one short, so the line that is left intact finishes the word.  With BOTH lines mutated mulvar_lazy
                             returns q for a multiple of q, and even that is absorbed by the fused product, whose inverse takes q as
                             the valid lazy word it is.  The pair is therefore held at the word mulvar_lazy returns.
"""
import numpy as np
import pytest

from helpers import harvey_cases as H
from oracle import cport as O

LOGNS = [1, 3, 6, 10]
_CASES = {}


def case(logn):
    """per limb: the forward, inverse and product families and the random vectors; built once, shared, never modified"""
    if logn not in _CASES:
        out = []
        for L in H.limbs(logn):
            c = dict(L=L, fwd=H.transform_families(L, False), inv=H.transform_families(L, True), prod=H.product_families(L),
                     rnd=H.random_vectors(L))
            for fam in (c["fwd"], c["inv"], c["prod"]):
                for member in fam:
                    for a in member[1:]:
                        a.setflags(write=False)
            out.append(c)
        _CASES[logn] = out
    return _CASES[logn]


def _oracle(L, vec, inverse):
    return (O.nwt_inverse if inverse else O.nwt_forward)(vec % np.uint64(L.q), L.q, L.rp)


@pytest.mark.parametrize("logn", LOGNS)
def test_moduli_are_the_ones_asked_for(logn):
    N = 1 << logn
    top, second, low = H.moduli(logn)
    assert [top, second] == sorted(O.gen_primes(max(N, 2), 61, 2), reverse=True)
    assert low >= 1 << 50 and low % (2 * N) == 1
    # nothing between 2^50 and `low` is a prime of the class
    assert not any(H.NT.is_prime(p) for p in range(((1 << 50) // (2 * N)) * 2 * N + 1, low, 2 * N) if p >= 1 << 50)


@pytest.mark.parametrize("logn", LOGNS)
def test_families_have_exactly_the_claimed_support(logn):
    for c in case(logn):
        L = c["L"]
        for inverse in (False, True):
            for name, vec, want, mask in c["inv" if inverse else "fwd"]:
                out = _oracle(L, vec, inverse)
                assert (out == want).all() and ((out != 0) == mask).all(), (logn, L.q, inverse, name)
                if name.startswith("lifted_"):
                    assert int((vec >= np.uint64(L.q)).sum()) == (L.N + 2) // 3
                    assert L.N < 7 or int(vec.max()) > (1 << 64) - 1 - L.q        # (the third lifted word is the largest of its class)
        for name, a, b, want in c["prod"]:
            assert (O.polymul_ntt(a, b, L.psi, L.q) == want).all(), (logn, L.q, name)
            A, B = _oracle(L, a, False), _oracle(L, b, False)
            meet = int(((A != 0) & (B != 0)).sum())
            if name.startswith("disjoint"):
                assert meet == 0 and not want.any()
            elif name == "meet_one_slot":
                assert meet == 1 and want.all()               # one slot of the spectrum: no coefficient vanishes
            else:
                j = int(name.split("_")[1])
                zeros = np.flatnonzero(a == 0)
                assert zeros.size and (want[(zeros + j) % L.N] == 0).all() and int((want == 0).sum()) == zeros.size
                i = int(np.flatnonzero(a)[-1])                # a coefficient that wraps comes back negated
                assert (i + j >= L.N) == (L.N >= 4)          # (2^1: a = (a_0, 0), nothing wraps)
                if i + j >= L.N:
                    assert int(want[i + j - L.N]) == L.q - int(a[i])


@pytest.mark.parametrize("logn", [4, 5, 12, 13])
def test_natural_order_families_have_exactly_the_claimed_support(logn):
    Cy = H.CyclicLimb(logn)
    q = np.uint64(Cy.q)
    for inverse in (False, True):
        for name, vec, want, mask in H.natural_families(Cy, inverse):
            out = (O.intt_cyclic if inverse else O.ntt_cyclic)(vec % q, Cy.q, Cy.g)
            assert (out == want).all() and ((out != 0) == mask).all(), (logn, inverse, name)
            # the n-th root convention with w = g^((q-1)/N) is the same transform
            assert (H.nthroot(vec % q, Cy, inverse) == want).all(), (logn, inverse, name)


@pytest.mark.parametrize("logn", LOGNS)
def test_vectorised_lazy_forward_is_the_models(logn):
    for c in case(logn):
        L = c["L"]
        for name, vec, *_ in c["fwd"]:
            if not name.startswith("lifted_"):
                for stages in sorted({0, 1, logn - 1, logn}):
                    assert H.lazy_forward_np(L, vec, stages).tolist() == H.Model(L).forward_lazy([int(x) for x in vec], stages), (name, stages)


def _run(M, c, what):
    """[(name, got == want)] of one model over one kind of family"""
    out = []
    for name, *arrays in c[what]:
        if what == "prod":
            a, b, want = arrays
            got = M.polymul(a, b)
        else:
            vec, want, _ = arrays
            got = (M.inverse if what == "inv" else M.forward)(vec)
        out.append((name, got == want.tolist()))
    return out


def _run_random(M, c, what):
    L = c["L"]
    if what == "prod":
        return all(M.polymul(a, b) == O.polymul_ntt(a, b, L.psi, L.q).tolist() for a, b in zip(c["rnd"][::2], c["rnd"][1::2]))
    return all((M.inverse if what == "inv" else M.forward)(v) == _oracle(L, v, what == "inv").tolist() for v in c["rnd"])


@pytest.mark.parametrize("logn", LOGNS)
def test_true_model_equals_the_oracle_and_meets_the_equalities(logn):
    for c in case(logn):
        L = c["L"]
        for what in ("fwd", "inv", "prod"):
            M = H.Model(L)
            assert all(ok for _, ok in _run(M, c, what)), (logn, L.q, what)
            ev = dict(M.events)
            assert M.events["range"] == 0
            if logn >= 6:
                need = {"fwd": ("fold_eq", "final_q", "final_2q"), "inv": ("sum_eq", "final_q"), "prod": ("barrett_q",)}[what]
                assert all(ev.get(k, 0) >= 1 for k in need), (logn, L.q, what, ev)
            R = H.Model(L)
            assert _run_random(R, c, what), (logn, L.q, what)
            assert all(R.events[k] == 0 for k in H.EQUALITIES + ("range",)), (logn, L.q, what, dict(R.events))


# mutant -> the families whose OUTPUT WORDS must show it
CAUGHT_BY_WORDS = {"fwd_fold": ("fwd",), "canon1": ("fwd",), "canon2": ("fwd", "inv", "prod")}


@pytest.mark.parametrize("logn", LOGNS)
@pytest.mark.parametrize("site", sorted(CAUGHT_BY_WORDS))
def test_mutants_the_words_show(logn, site):
    """no random vector notices the mutant; at least one family member of every listed kind gives a wrong word -- and the wrong word
    is q where the oracle has 0.  2^1: the forward fold cannot be reached from canonical words in one stage (X < q), so that mutant is
    the true model there; every other requirement holds at every size."""
    for c in case(logn):
        L = c["L"]
        for what in ("fwd", "inv", "prod"):
            assert _run_random(H.Model(L, site), c, what), (logn, L.q, site, what)
        for what in CAUGHT_BY_WORDS[site]:
            caught = [name for name, ok in _run(H.Model(L, site), c, what) if not ok]
            if site == "fwd_fold" and logn < 3:
                assert caught == []
                continue
            assert caught, (logn, L.q, site, what)
            if site == "fwd_fold":
                assert caught == ["fold_tail"]
    if site == "fwd_fold" and logn >= 3:
        for c in case(logn):
            L = c["L"]
            name, vec, want, _ = c["fwd"][-1]
            got = H.Model(L, site).forward(vec)
            assert name == "fold_tail" and [i for i in range(L.N) if got[i] != int(want[i])] == [1] and got[1] == L.q and want[1] == 0


@pytest.mark.parametrize("logn", LOGNS)
def test_inverse_sum_mutant_breaks_the_range_and_never_a_word(logn):
    """(the module docstring has the argument) equal words on every family and every random vector; the operand range [0, 2q) broken
    on the families from 2^3 on, never on a random vector"""
    for c in case(logn):
        L = c["L"]
        for what in ("inv", "prod"):
            M = H.Model(L, "inv_sum")
            assert all(ok for _, ok in _run(M, c, what)), (logn, L.q, what)
            assert (M.events["range"] >= 1) == (logn >= 3), (logn, L.q, what, dict(M.events))
            R = H.Model(L, "inv_sum")
            assert _run_random(R, c, what) and R.events["range"] == 0


@pytest.mark.parametrize("logn", LOGNS)
def test_barrett_fix_ups_absorb_each_other(logn):
    """(the module docstring has the argument) either fix-up alone as ``>``: the same words, in the product and in mulvar_lazy
    itself.  Both: mulvar_lazy returns q on the multiples of q the disjoint spectra give it -- that is what the product families
    catch -- and the fused product still returns the oracle's words."""
    for c in case(logn):
        L = c["L"]
        name, a, b, want = c["prod"][0]
        assert name == "disjoint_halves"
        fa, fb = (H.lazy_forward_np(L, v, logn).tolist() for v in (a, b))
        exact = [x * y % L.q for x, y in zip(fa, fb)]
        assert not any(exact)
        for mutant in ((), "barrett1", "barrett2"):
            M = H.Model(L, mutant)
            assert [M.mulvar_lazy(x, y) for x, y in zip(fa, fb)] == exact
            assert all(ok for _, ok in _run(H.Model(L, mutant), c, "prod")) and _run_random(H.Model(L, mutant), c, "prod")
        both = H.Model(L, ("barrett1", "barrett2"))
        got = [both.mulvar_lazy(x, y) for x, y in zip(fa, fb)]
        assert set(got) <= {0, L.q} and got.count(L.q) == both.events["barrett_q"] >= 1, (logn, L.q)
        assert all(ok for _, ok in _run(H.Model(L, ("barrett1", "barrett2")), c, "prod"))
