"""The natural-order transform (launch_gs_t: the inverse-structured network on bit-reversed input with a cyclic table) on inputs built
for its own table (tests/helpers/gs_worst_case.py), without a GPU: the helper against the oracle, the route's fold schedule as its
templates fix it against the helper's restatement and under the exact-fraction walk, and the emulation of its two launches -- the
gathering row pass and the column pass, tests/emu/emu_ntt.cpp emu_ntt_gs -- with the live range tracker on every designed vector."""
import ctypes as C

import numpy as np
import pytest

from oracle import cport as O
from test_emu_passes import emu  # noqa: F401  (the emulation library fixture)
from test_ntt_worst_case import Q_WALK, _schedule, _walk_inverse
from helpers import gs_worst_case as G
from helpers import ntt_worst_case as W

EMU_SIZES = [5, 9, 12, 13, 14, 16, 17]
p64 = C.POINTER(C.c_uint64)
_LIMBS = {}


def limb(logn, bits, inverse):
    key = (logn, bits, bool(inverse))
    if key not in _LIMBS:
        _LIMBS[key] = G.GsLimb(*key)
    return _LIMBS[key]


# ------------------------------------------------------------------ the helper against the oracle
@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("bits", [50, 30])
@pytest.mark.parametrize("logn", [5, 9, 13])
def test_staged_network_is_the_oracles_cyclic_transform(logn, bits, inverse):
    L = limb(logn, bits, inverse)
    assert L.q < 1 << bits and (L.q - 1) % L.N == 0 and not any(G._is_prime(p) for p in range(L.q + L.N, 1 << bits, L.N))
    assert pow(L.g, (L.q - 1) // 2, L.q) == L.q - 1 and all(pow(x, (L.q - 1) // 2, L.q) == 1 for x in range(2, L.g))
    assert (O.modmul(L.tw, L.tw_inv, L.q) == 1).all()
    x = G.random_vector(L)
    assert (G.network(L, x) == L.oracle(x)).all()
    other = limb(logn, bits, not inverse)
    assert (G.network(other, G.network(L, x)) == x).all()


@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("bits", [50, 30])
@pytest.mark.parametrize("logn", [5, 9, 13])
def test_every_pulse_is_c_everywhere_after_its_stages(logn, bits, inverse):
    L = limb(logn, bits, inverse)
    c = W.pulse_residue(L.q)
    for t in range(logn):
        vec, reach, pair = G.natural_pulse(L, t)
        assert (G.stages(L, vec[L.perm], t) == c).all(), t
        assert reach >= c / L.q and pair >= 2 * c / L.q
    names = [n for n, *_ in G.families(L)]
    assert names == [f"pulse{t}" for t in range(logn)] + ["all_qm1", "half"] + [f"alt{lg}" for lg in range(logn)] + ["spikes", "near_q"]
    # alt{lg} lands on the network's pair structure: in network order it is blocks of 2^lg, so the first lg stages pair equal words
    for name, vec, *_ in G.families(L):
        if name.startswith("alt"):
            lg = int(name[3:])
            net = vec[L.perm]
            assert (net == np.where((np.arange(L.N) >> lg) % 2 == 0, 0, L.q - 1)).all()


# ------------------------------------------------------------------ the schedule this route really gets
def test_route_schedule_is_the_plan_family(emu):
    """GsPasses::First / Second dumped from their template arguments (form 5): canonical words in, entry bound q, the lazy
    per-register plan, lazy hand-off between two launches, the scale folded into the last stage -- step for step the schedule of
    Passes<.., true, GEO> (form 0), which is what the helper's reach model assumes (G.GS_FORM)."""
    assert G.GS_FORM == "plan"
    for logn in range(1, 21):
        got = _schedule(emu, 5, logn, 1)
        if logn < 5:
            assert got is None
            continue
        assert _schedule(emu, 5, logn, 0) is None
        assert got == _schedule(emu, 0, logn, 1), logn
        assert len(got) == (2 if logn >= 13 else 1)
        assert got[0]["kind"] == 0 and got[0]["in_mode"] == 0 and got[0]["lazy"] == 1 and got[0]["in8"] == 8
        assert got[-1]["out_mode"] == 0 and got[-1]["steps"][-1][4] == 1
        assert sum(fold for p in got for *_, fold in p["steps"]) == 1
        if len(got) == 2:
            assert got[0]["out_mode"] == 1 and got[1]["kind"] == 1 and got[1]["in_mode"] == 1 and got[1]["lazy"] == 1
        steps = [K for q in got for K, *_ in q["steps"]]
        assert [(g, K) for g, K, *_ in W.inverse_schedule(logn, G.GS_FORM)] == [(sum(steps[:i]), K) for i, K in enumerate(steps)]


def test_route_schedule_walk(emu):
    """the exact-fraction walk of tests/test_ntt_worst_case.py over this route's dumped schedule at Q_WALK: the bound is carried from
    step to step and across the hand-off by the walk, and no register or pair passes 8 q"""
    assert Q_WALK == (1 << 50) - 1
    for logn in range(5, 21):
        top = _walk_inverse(emu, _schedule(emu, 5, logn, 1), None, (logn, "gs"))
        assert top <= 8
        if logn in (12, 16, 20):
            assert top == 8                        # a first step of four stages: canonical words reach the limit, 1, 2, 4, 8


# ------------------------------------------------------------------ the two launches under the tracker
def _gs(emu, L, vec):
    emu.emu_ntt_gs.restype = C.c_int
    emu.emu_ntt_gs.argtypes = [p64, p64, C.c_int, C.c_uint64, p64, C.c_uint64]
    emu.emu_max_pair.restype = C.c_double
    src = np.ascontiguousarray(vec, dtype=np.uint64)
    dst = np.zeros_like(src)
    tw = np.ascontiguousarray(L.tw)
    assert emu.emu_ntt_gs(dst.ctypes.data_as(p64), src.ctypes.data_as(p64), L.logn, L.q, tw.ctypes.data_as(p64), L.scale) == 0
    return dst, emu.emu_max_ratio(), emu.emu_max_pair()


@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("bits", [50, 30])
@pytest.mark.parametrize("logn", EMU_SIZES)
def test_tracked_emulation_on_designed_vectors(emu, logn, bits, inverse):
    """Words equal the oracle; no register and no pair above 8 q; every vector reaches what its model predicts (exactly that where
    the model is exact); and the designed set reaches further than a seeded random vector -- a family that steers nothing would not."""
    L = limb(logn, bits, inverse)
    best = best_pair = 0.0
    for name, vec, reach, pair, exact in G.families(L):
        got, mx, mp = _gs(emu, L, vec)
        what = (name, logn, bits, inverse)
        assert (got == L.oracle(vec)).all(), what
        assert mx <= 8.0 and mp <= 8.0, (what, mx, mp)
        assert mx >= reach - 1e-12 and mp >= pair - 1e-12, (what, mx, reach, mp, pair)
        if exact:
            assert abs(mx - reach) <= 1e-12 and abs(mp - pair) <= 1e-12, (what, mx, reach, mp, pair)
        best, best_pair = max(best, mx), max(best_pair, mp)
    x = G.random_vector(L)
    got, rx, rp = _gs(emu, L, x)
    assert (got == L.oracle(x)).all()
    assert rx <= 8.0 and rp <= 8.0
    assert best > rx and best_pair > rp, (logn, bits, inverse, best, rx, best_pair, rp)
    print(f"natural-order reach 2^{logn} {bits}-bit {'inverse' if inverse else 'forward'}: designed {best:.4f} q (pair {best_pair:.4f}), "
          f"random {rx:.4f} q (pair {rp:.4f})")


def test_out_of_range_words_enter_as_their_residues(emu):
    """the gathering launch reduces a word at or above q on the way in, like every canonical load"""
    L = limb(9, 50, 0)
    x = G.random_vector(L)
    y = x.copy()
    y[3] += np.uint64(L.q)
    y[100] = np.uint64(2**64 - 1)
    y[511] = np.uint64(L.q)
    got, mx, mp = _gs(emu, L, y)
    assert (got == L.oracle(y % np.uint64(L.q))).all() and mx <= 8.0 and mp <= 8.0
