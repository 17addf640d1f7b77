"""The census of tests/test_harvey_cases.py taken on the REAL templates: the families of tests/helpers/harvey_cases.py through the CPU
emulation of the HIP passes (tests/emu/emu_ntt.cpp), with the integer path routed through TrackU64 -- ArithU64 itself, every operand
watched.  Per schedule (single pass, two launches, LDS-resident, fused) and per modulus: the words equal the oracle, every output is
below q, no operand leaves its documented range (below 4q forward, below 2q inverse), and the equalities the Python model requires
are met -- X == 2q at the forward fold, final words q and 2q, X + Y == 2q at the inverse sum, final word q.  Which events are
required comes from the model and the oracle (tests/test_harvey_cases.py), never from the emulated code.

No schedule is exempt from a requirement: the first forward stage cannot meet the fold from canonical input, but every schedule has
later stages, and the counts below are per whole transform."""
import ctypes as C

import numpy as np
import pytest

from helpers import harvey_cases as H
from helpers import ntt_worst_case as W
from helpers.emu_build import build_emu
from oracle import cport as O

p64 = C.POINTER(C.c_uint64)
EVENTS = ("fold_eq", "sum_eq", "final_q", "final_2q", "final_3q", "shoup_hi", "barrett_q", "range")     # emu_ntt.cpp's EV_ order
# (logn, schedule name, emu_ntt's fused_dist argument)
SCHEDULES = [(logn, "single_pass", 0) for logn in (3, 9, 12)] + [(logn, "two_launch", 0) for logn in (13, 14, 16)]
SCHEDULES += [(logn, "resident", -2) for logn in (13, 14)] + [(logn, "fused", 3) for logn in (13, 14, 16)]


@pytest.fixture(scope="module")
def emu():
    L = build_emu("libemu_ntt.so", ["emu_ntt.cpp"], ("modarith.hpp", "ntt_core.hpp", "ntt_plan.hpp", "ntt_fused.hpp"))
    L.emu_ntt.restype = C.c_int
    L.emu_ntt.argtypes = [p64, C.c_int, C.c_int, C.c_int, C.c_int, p64, p64, C.c_int, C.c_int]
    L.emu_u64_events.restype = None
    L.emu_u64_events.argtypes = [p64]
    L.emu_u64_mulvar_lazy.restype = None
    L.emu_u64_mulvar_lazy.argtypes = [p64, p64, p64, C.c_size_t, C.c_uint64]
    return L


def _events(emu):
    out = np.zeros(len(EVENTS), dtype=np.uint64)
    emu.emu_u64_events(out.ctypes.data_as(p64))
    return dict(zip(EVENTS, (int(x) for x in out)))


def _transform(emu, L, batch, inverse, dist):
    """the batch [P][N] of one limb through the integer path: (words, events of the call)"""
    d = np.ascontiguousarray(batch, dtype=np.uint64).copy()[:, None, :]
    q = np.array([L.q], dtype=np.uint64)
    rp = np.ascontiguousarray(L.rp, dtype=np.uint64)
    rc = emu.emu_ntt(d.ctypes.data_as(p64), L.logn, 1 if inverse else 0, d.shape[0], 1, q.ctypes.data_as(p64), rp.ctypes.data_as(p64), 1, dist)
    assert rc == 0, rc
    return d[:, 0, :], _events(emu)


_LIMBS = {}


def _limbs(logn):
    if logn not in _LIMBS:
        _LIMBS[logn] = [(L, H.transform_families(L, False), H.transform_families(L, True)) for L in H.limbs(logn)]
    return _LIMBS[logn]


@pytest.mark.parametrize("logn,schedule,dist", SCHEDULES, ids=[f"{a}-{b}" for a, b, _ in SCHEDULES])
def test_families_through_every_schedule(emu, logn, schedule, dist):
    for L, fwd, inv in _limbs(logn):
        for inverse, fam in ((False, fwd), (True, inv)):
            names = [n for n, *_ in fam]
            got, ev = _transform(emu, L, np.stack([v for _, v, *_ in fam]), inverse, dist)
            what = (logn, schedule, L.q, inverse, ev)
            bad = [n for n, g, (_, _, want, _) in zip(names, got, fam) if not (g == want).all()]
            assert bad == [], what
            assert (got < np.uint64(L.q)).all(), what
            assert ev["range"] == 0, what
            need = ("sum_eq", "final_q") if inverse else ("fold_eq", "final_q", "final_2q")
            assert all(ev[k] >= 1 for k in need), what
        # the forward fold's own family: the pair (2q, 0) reaches the last stage in this schedule too
        name, vec, want, _ = fwd[-1]
        assert name == "fold_tail"
        got, ev = _transform(emu, L, vec[None, :], False, dist)
        assert (got[0] == want).all() and ev["fold_eq"] >= 1 and ev["range"] == 0


@pytest.mark.parametrize("logn,schedule,dist", SCHEDULES, ids=[f"{a}-{b}" for a, b, _ in SCHEDULES])
def test_random_and_soak_vectors_stay_in_range_and_meet_nothing(emu, logn, schedule, dist):
    """the range assertions on the soak patterns (all q - 1, alternating blocks, spikes, words next to q) and on random vectors, on
    which no comparison meets equality: that is why the suite could not tell >= from > before"""
    for L, _, _ in _limbs(logn):
        soak = np.stack([v for _, v, *_ in W.soak_patterns(L)])
        rnd = np.stack(H.random_vectors(L, count=3))
        for inverse in (False, True):
            ref = O.nwt_inverse if inverse else O.nwt_forward
            for batch, random in ((soak, False), (rnd, True)):
                got, ev = _transform(emu, L, batch, inverse, dist)
                assert all((g == ref(v, L.q, L.rp)).all() for g, v in zip(got, batch)), (logn, schedule, L.q, inverse, random)
                assert (got < np.uint64(L.q)).all() and ev["range"] == 0, (logn, schedule, L.q, inverse, random, ev)
                if random:
                    assert all(ev[k] == 0 for k in H.EQUALITIES), (logn, schedule, L.q, inverse, ev)


@pytest.mark.parametrize("logn", [3, 9, 12, 13])
def test_barrett_step_on_exact_multiples_of_q(emu, logn):
    """ArithU64::mulvar_lazy as the fused product calls it, on the lazy spectra of the product families: where the supports are
    disjoint every product is a nonzero multiple of q unless a factor is the word 0, the quotient estimate is one short, and the
    fix-up decides the word.  Canonical words, equal to the exact product, the event counted as often as Python integers say."""
    for L in H.limbs(logn):
        for name, a, b, _ in H.product_families(L):
            fa, fb = H.lazy_forward_np(L, a, logn), H.lazy_forward_np(L, b, logn)
            assert int(fa.max()) < 4 * L.q and int(fb.max()) < 4 * L.q
            c = np.zeros(L.N, dtype=np.uint64)
            before = _events(emu)
            emu.emu_u64_mulvar_lazy(c.ctypes.data_as(p64), fa.ctypes.data_as(p64), fb.ctypes.data_as(p64), L.N, L.q)
            after = _events(emu)
            exact = [int(x) * int(y) for x, y in zip(fa, fb)]
            assert c.tolist() == [x % L.q for x in exact], (logn, L.q, name)
            ratio = (1 << 128) // L.q
            left_q = sum(1 for x in exact if x - ((x * ratio) >> 128) * L.q == L.q)
            assert after["barrett_q"] - before["barrett_q"] == left_q and after["range"] == before["range"], (logn, L.q, name)
            if name.startswith("disjoint"):
                assert not c.any() and left_q == sum(1 for x in exact if x) >= 1, (logn, L.q, name)
