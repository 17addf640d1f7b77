"""The cyclic transform's oracle pinned, without a GPU, for every small and unusual (modulus, root) pair the GPU tests use
(tests/helpers/cyclic_cases.py), and the reason the natural-order launches cannot serve all of them."""
import numpy as np
import pytest

from oracle import cport as O
from helpers import cyclic_cases as K
from helpers import gs_worst_case as G


@pytest.mark.parametrize("mod,root,logns", K.CASES, ids=[f"{m}-{r}" for m, r, _ in K.CASES])
def test_oracle_is_the_plain_python_definition(mod, root, logns):
    for logn in logns:
        for name, v in K.inputs(mod, logn):
            if logn >= 16 and name not in ("random", "out_of_range"):
                continue                                  # (half a second of plain Python per vector)
            assert O.ntt_cyclic(v, mod, root).tolist() == K.plain_ntt(v.tolist(), mod, root), (mod, logn, name)
            assert O.intt_cyclic(v, mod, root).tolist() == K.plain_intt(v.tolist(), mod, root), (mod, logn, name)


def test_which_cases_have_a_root_tower():
    for mod, root, logns in K.CASES:
        for logn in logns:
            want = (mod, root) in K.TOWER or (mod, logn) == (3, 1)
            assert K.has_tower(mod, root, logn) == want, (mod, root, logn)
            assert K.has_tower(mod, pow(root, mod - 2, mod), logn) == want      # the inverse call's root


@pytest.mark.parametrize("mod,root,logn", [(1 << 20, 3, 9), (998244353, 4, 5), (3 * 65537, 5, 5), (65537, 3, 5), (257, 3, 8)])
def test_transposed_network_needs_a_root_tower(mod, root, logn):
    """The natural-order launches run the transposed network (helpers/gs_worst_case.py network): it is the definition's transform
    wherever the roots form a tower (a sufficient condition: some towerless sets coincide too), and is NOT for 2^20 at 2^9 on a random
    vector -- the input that showed it.  The forward network with the same table is the definition relabelled by the bit reversal,
    tower or not: the route fhe_ntt_cyclic takes for every towerless call."""
    L = G.GsLimb.__new__(G.GsLimb)
    L.logn, L.N, L.q, L.scale, L.perm = logn, 1 << logn, mod, 1, G.bitrev_perm(logn)
    L.tw = G.cyclic_table(mod, logn, root)
    v = dict(K.inputs(mod, logn))["random"]
    want = O.ntt_cyclic(v, mod, root)
    same = (G.network(L, v) == want).all()
    assert same or not K.has_tower(mod, root, logn)
    if mod == 1 << 20:
        assert not same
    assert (O.nwt_forward(v, mod, L.tw)[L.perm] == want).all()


def test_fourstep_reference_differs_from_the_network_for_a_root_that_generates_nothing():
    """four_step_ntt is the direct DFT with w = g^((mod-1)/N).  For the quadratic residue 4 modulo 998244353, w^(N/2) = +1: its output
    has period N/2 and is NOT the cyclic network's, which the engine runs -- so fhe_fourstep_create refuses such a plan (the GPU
    test expects the status).  For a generator the two are the same words."""
    mod = 998244353
    for logn, n1 in ((5, 4), (9, 16)):
        v = dict(K.inputs(mod, logn))["random"]
        N = 1 << logn
        assert not K.has_tower(mod, 4, logn) and K.has_tower(mod, 3, logn)
        assert (O.four_step_ntt(v, n1, N // n1, mod, 3) == O.ntt_cyclic(v, mod, 3)).all()
        y = O.four_step_ntt(v, n1, N // n1, mod, 4)
        assert not (y == O.ntt_cyclic(v, mod, 4)).all()
        assert (y[:N // 2] == y[N // 2:]).all()
