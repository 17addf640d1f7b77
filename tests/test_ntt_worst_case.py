"""The FP64 transform's lazy range on inputs that reach for it (tests/helpers/ntt_worst_case.py), without a GPU: the helper against
the oracle's stage-wise reference, an exact-fraction walk of every fold schedule the templates produce, and the emulation with a
live tracker (tests/emu/emu_ntt.cpp TrackF64) on the designed vectors."""
import ctypes as C
from fractions import Fraction as Fr

import numpy as np
import pytest

from oracle import cport as O
from test_emu_passes import emu, _run  # noqa: F401  (the emulation library fixture and its caller)
from helpers import ntt_worst_case as W

Q_WALK = (1 << 50) - 1                       # the walk's modulus: the largest the FP64 path admits
GROW = Fr(Q_WALK, 1 << 52)                   # a product's share of its input: |a w - k q| <= q/2 + |a| q 2^-52
SLACK = Fr(1, 1 << 40)                       # an ulp of the quotient on a fold or a product
EMU_SIZES = [4, 9, 12, 13, 14, 16, 17]
KIND = {"plain": "plan", "unitlist": "plan", "fused1": "mask", "fused3": "mask", "resident": "resident"}
FORMS = {"plain": 0, "fused1": 1, "fused3": 3, "resident": -2, "packed": -3, "unitlist": -1}


@pytest.fixture(scope="module")
def limbs():
    cache = {}

    def get(logn, bits):
        if (logn, bits) not in cache:
            cache[logn, bits] = W.Limb(logn, bits)
        return cache[logn, bits]
    return get


def _forms(logn, inverse):
    f = ["plain"]
    if 13 <= logn <= 17:
        f += ["fused1", "fused3"]
    if logn in (13, 14):
        f.append("resident")
    if logn == 16 and not inverse:
        f.append("packed")
    if logn in (12, 13):
        f.append("unitlist")
    return f


# ------------------------------------------------------------------ the helper itself
def test_stage_wise_reference_composes_to_the_transform():
    L = W.Limb(9, 50)
    rng = np.random.default_rng(1)
    a = rng.integers(0, L.q, L.N, dtype=np.uint64)
    f = a
    for s in range(L.logn):
        f = O.nwt_forward_stage(f, s, L.q, L.rp)
    assert (f == O.nwt_forward(a, L.q, L.rp)).all()
    g = f
    for s in range(L.logn - 1, -1, -1):
        g = O.nwt_inverse_stage(g, s, L.q, L.rp_inv)
    assert (g == O.modmul(a, np.full(L.N, L.N % L.q, dtype=np.uint64), L.q)).all()      # the unscaled inverse: N a


def test_model_of_the_arithmetic_is_exact_on_its_own_terms():
    q = W.prime_below(50, 16)
    rng = np.random.default_rng(2)
    for _ in range(200):
        a, w = int(rng.integers(-8 * q, 8 * q)), int(rng.integers(1, q))
        r = W.model_mulmod(a, w, q)
        assert (r - a * w) % q == 0 and abs(r) <= q * (Fr(1, 2) + abs(a) * Fr(1, 1 << 52)) + 1
        x = W.model_reduce(a, q)
        assert (x - a) % q == 0 and abs(x) <= q // 2 + 1


@pytest.mark.parametrize("logn", [4, 9, 13, 16, 18])
@pytest.mark.parametrize("bits", [50, 30])
def test_helper_vectors_reach_the_dictated_states(limbs, logn, bits):
    L = limbs(logn, bits)
    q = L.q
    for s0, K, canonical in W.forward_stretches(logn) + (W.forward_stretches(16, canonical_at=(8,)) if logn == 16 else []):
        vec, state, reach, tops = W.forward_ladder(L, s0, K, canonical)
        got = vec
        for s in range(s0):
            got = O.nwt_forward_stage(got, s, q, L.rp)
        assert (got == state).all(), (s0, K)
        # and in exact integers, block by block: register 0 climbs by the dictated words' products, each the residue below q/2
        for p, lo, top in tops:
            base = (p << (logn - s0)) | lo
            x = int(state[base])
            for i in range(K):
                y = int(state[base + ((1 << (K - 1 - i)) << (logn - s0 - K))])
                h = y * int(L.rp[(1 << (s0 + i)) + (p << i)]) % q
                assert h == 0 or 0 <= (q - 1) // 2 - h < 64
                x += h
            assert x == top, (s0, K, p, lo)
        assert reach == max(t for _, _, t in tops) / q
    c = W.pulse_residue(q)
    for t in range(logn):
        vec, reach, pair = W.inverse_pulse(L, t)
        got = vec
        for v in range(t):
            got = O.nwt_inverse_stage(got, logn - 1 - v, q, L.rp_inv)
        assert (got == c).all(), t
        vec, reach = W.forward_pulse(L, t)
        got = vec
        for s in range(t):
            got = O.nwt_forward_stage(got, s, q, L.rp)
        assert (got == c).all(), t


def test_helper_restates_the_inverse_schedule(emu):
    """the helper's own statement of the inverse fold schedule (it imports nothing) against what the templates produce; form 5 is the
    natural-order route (GsPasses), whose designed inputs (helpers/gs_worst_case.py) lean on the same "plan" restatement"""
    u32p = C.POINTER(C.c_uint32)
    emu.emu_inv_lazy_plan.restype = C.c_int
    emu.emu_inv_lazy_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, u32p, u32p, C.POINTER(C.c_int)]
    for logn in range(1, 21):
        for form, kind in ((0, "plan"), (1, "mask"), (2, "resident"), (5, "plan")):
            passes = _schedule(emu, form, logn, 1)
            if passes is None:
                continue
            want = []
            g = 0
            for p in passes:
                for K, mask, in8, ex8, fold in p["steps"]:
                    if p["lazy"]:
                        before = (C.c_uint32 * K)()
                        ae, out8 = C.c_uint32(), C.c_int()
                        assert emu.emu_inv_lazy_plan(K, in8, ex8, fold, before, C.byref(ae), C.byref(out8)) == 0
                        want.append((g, K, [before[v] for v in range(K)], ae.value, bool(fold)))
                    else:
                        want.append((g, K, [((1 << (1 << K)) - 1) if (mask >> v) & 1 else 0 for v in range(K)], 0, bool(fold)))
                    g += K
            assert W.inverse_schedule(logn, kind) == want, (logn, kind)


# ------------------------------------------------------------------ reach floors: conditions on the helper's own model
def test_reach_floors(limbs):
    """Forward: the issue's floors.  Inverse: the issue's floor is a pair sum of 7.9 q in front of a butterfly at some stage of every
    register step the plan folds.  The model attains it only in the FIRST step (canonical words: 8 (q - 1)); in a later step it can
    vouch for no more than the registers the plan folds, which hold +c exactly: 2 c = 1.0 q where a pair is folded at the step's
    last stage or only one of the pair is folded, 4 c = 2.0 q where both are folded one stage earlier.  Everything else a later step
    holds is a sum whose representative depends on the history, which the model does not dictate (the emulation's tracker sees 4 q to
    7.2 q there).  Those attained figures are asserted; both sets are in DESIGN.md."""
    for bits in (50, 30):
        L = limbs(16, bits)
        assert W.forward_ladder(L, 0, 5, True)[2] >= 3.4          # five stages from canonical words: (q-1) + 5 h
        assert W.forward_ladder(L, 5, 6, False)[2] >= 3.4         # six stages after a fold: (q-1)/2 + 6 h
        for logn in (4, 9, 12, 13, 16, 17, 18):
            L = limbs(logn, bits)
            sched = W.inverse_schedule(logn, "plan")
            if sched[0][1] >= 3:
                assert W.all_qm1_inverse_reach(L, "plan")[1] >= 7.9                 # the issue's figure, first step
                assert W.inverse_pulse_reach(L, 0, "plan")[1] >= 3.99               # canonical c: c, 2c, 4c on the sum branch
            for g, K, before, at_exit, scaled in sched:
                if not any(before):
                    continue
                best = max(W.inverse_pulse_reach(L, t, "plan")[1] for t in range(g, g + K))
                # both registers of a pair folded before the step's last stage: +c, +c, then 2c + 2c
                both_early = any((before[v] >> r) & 1 and (before[v] >> (r + (1 << v))) & 1 for v in range(K - 1) for r in range(1 << K)
                                 if not (r >> v) & 1)
                assert best >= (1.99 if both_early or g == 0 else 0.99), (logn, g, K, best)


# ------------------------------------------------------------------ exact-fraction walk of every fold schedule
def _schedule(emu, form, logn, inverse):
    emu.emu_fold_schedule.restype = C.c_int
    emu.emu_fold_schedule.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]
    buf = (C.c_int * 256)()
    n = emu.emu_fold_schedule(form, logn, inverse, buf, 256)
    if n < 0:
        return None
    assert n <= 256
    v, passes, i = list(buf[:n]), [], 0
    while i < n:
        kind, nstep, in_mode, out_mode, lazy, in8 = v[i:i + 6]
        i += 6
        steps = [tuple(v[i + 5 * j:i + 5 * j + 5]) for j in range(nstep)]
        i += 5 * nstep
        passes.append(dict(kind=kind, in_mode=in_mode, out_mode=out_mode, lazy=lazy, in8=in8, steps=steps))
    return passes


def _walk_forward(passes, where):
    """B' = B (1 + q 2^-52) + 1/2 for both outputs of a butterfly on registers bounded by B; a fold leaves 1/2.  Returns the
    largest bound met anywhere: before a butterfly, before a fold and on the words a pass leaves."""
    B, top = None, Fr(0)
    for p in passes:
        if p["in_mode"] == 0:
            B = Fr(1)
        assert B is not None
        grow = p.get("grow", GROW)
        for K, mask, _, _, _ in p["steps"]:
            for u in range(K):
                assert B < 8, (where, float(B))
                if (mask >> u) & 1:
                    B = Fr(1, 2) + SLACK
                top = max(top, B)
                B = B * (1 + grow) + Fr(1, 2)
                assert B < 8, (where, float(B))
                top = max(top, B)
    return top


def _walk_inverse(emu, passes, entry, where):
    """Per register, as test_inverse_lazy_range_plan_is_sound models a Gentleman-Sande stage, but with the bound carried from step
    to step and from launch to launch by this walk, not taken from what the kernels declare."""
    u32p = C.POINTER(C.c_uint32)
    emu.emu_inv_lazy_plan.restype = C.c_int
    emu.emu_inv_lazy_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, u32p, u32p, C.POINTER(C.c_int)]
    carried, top = None, Fr(0)
    for p in passes:
        if p["in_mode"] == 0:
            carried = Fr(1)
        elif carried is None:
            carried = entry
        for K, mask, in8, ex8, fold in p["steps"]:
            R = 1 << K
            b = [carried] * R
            at_exit = 0
            if p["lazy"]:
                before = (C.c_uint32 * K)()
                ae, out8 = C.c_uint32(), C.c_int()
                assert emu.emu_inv_lazy_plan(K, in8, ex8, fold, before, C.byref(ae), C.byref(out8)) == 0
                masks, at_exit = [before[v] for v in range(K)], ae.value
            else:
                masks = [((1 << R) - 1) if (mask >> v) & 1 else 0 for v in range(K)]
            for v in range(K):
                u = K - 1 - v
                half = R >> (u + 1)
                for r in range(R):
                    assert b[r] <= 8, (where, float(b[r]))     # (8 itself only as 8 (q - 1), the sum of canonical words)
                    if (masks[v] >> r) & 1:
                        b[r] = Fr(1, 2) + SLACK
                for blk in range(1 << u):
                    for j in range(half):
                        i0 = blk * 2 * half + j
                        i1 = i0 + half
                        ssum = b[i0] + b[i1]
                        assert ssum <= 8, (where, K, v, i0, i1, float(ssum))
                        top = max(top, ssum)
                        prod = Fr(1, 2) + ssum * GROW + SLACK
                        b[i0] = prod if (fold and u == 0) else ssum
                        b[i1] = prod
            for r in range(R):
                assert b[r] <= 8, (where, float(b[r]))
                if (at_exit >> r) & 1:
                    b[r] = Fr(1, 2) + SLACK
            carried = max(b)
        assert carried < 8 or p["out_mode"] == 0 and carried <= 8, (where, float(carried))   # (a scaled last stage leaves products)
    return top


def test_forward_fold_schedule_walk(emu):
    """Every forward schedule the templates produce -- Passes (both launches), FusedPasses, ResidentPass, the product's middle
    launch (MidPasses) and the packed hand-off -- for 2^1 .. 2^20: no register at or above 8 q anywhere."""
    table = {}
    for logn in range(1, 21):
        seen = 0
        for form in (0, 1, 2, 4):
            passes = _schedule(emu, form, logn, 0)
            if passes is None:
                continue
            seen += 1
            table[logn, form] = _walk_forward(passes, (logn, form))
        # the product: first launch of Passes (two-launch sizes), then the middle launch's forward row pass
        first = _schedule(emu, 0, logn, 0)
        mid = _schedule(emu, 3, logn, 0)
        table[logn, 3] = _walk_forward((first[:1] if len(first) == 2 else []) + mid, (logn, 3))
        assert seen >= 1 + (13 <= logn <= 17) + (logn in (13, 14)) + (logn == 16)
    # the table DESIGN.md quotes: the largest bound a size meets
    assert float(table[4, 0]) < 5.4 and 7.1 < float(table[5, 0]) < 7.2 and 7.5 < float(table[11, 0]) < 7.6
    assert max(table.values()) == table[20, 0] == table[11, 0]
    # the stretches the helper aims its ladders at are the schedule's
    b = (C.c_int * 4)()
    emu.emu_f64_budgets(b)
    assert list(b) == [W.FWD_FIRST, W.FWD_NEXT, 2, 3]


def _regroup(p, steps, mask=None, **more):
    """the pass p with its stages grouped into other register steps (the fold mask is per stage: bit u = before stage u of the pass)"""
    if mask is None:
        mask, u0 = 0, 0
        for K, m, *_ in p["steps"]:
            mask |= m << u0
            u0 += K
    out, u0 = [], 0
    for K in steps:
        out.append((K, (mask >> u0) & ((1 << K) - 1), 0, 0, 0))
        u0 += K
    assert u0 == sum(K for K, *_ in p["steps"])
    return dict(p, steps=out, **more)


def test_key_switch_row_pass_walks(emu):
    """The two forward row passes the key switch's fused inner product builds outside the headers (ntt_kernels.hip), walked after the
    first launch of Passes.  k_ks_rowmac at 2^16 regroups the product's middle row pass into Steps<3, 3, 2> and keeps its mask
    (MidPasses::F::RED_SECOND), so the per-stage walk of form 3 is its walk; it is repeated here in that grouping.  RowMacLt takes its
    factors from LDS (RowTwLds): the quotient w * (1/q) is within 1.5 ulp, a product is bounded by 1/2 + 3 B / 8, and its mask
    red_every4 -- RESTATED here, the emulation cannot include a .hip file -- folds before stages 0, 4, 8, ... of the pass."""
    for logn in range(13, 21):
        first = _schedule(emu, 0, logn, 0)[:1]
        mid = _schedule(emu, 3, logn, 0)[0]
        steps = [K for K, *_ in mid["steps"]]
        PR = sum(steps)
        if logn == 16:
            assert PR == 8
            assert _walk_forward(first + [_regroup(mid, [3, 3, 2])], (logn, "rowmac")) == _walk_forward(first + [mid], (logn, 3))
        every4 = sum(1 << u for u in range(0, PR, 4))
        top = _walk_forward(first + [_regroup(mid, [3, 3, 2] if PR == 8 else steps, every4, grow=GROW * 3 / 2)], (logn, "RowTwLds"))
        assert top < 8
    # four stages from a fold under B' = B (1 + 3/8) + 1/2: 0.5, 1.19, 2.13, 3.43, 5.22 -- the pass itself never passes 5.3
    tail = _walk_forward([dict(in_mode=0, out_mode=1, steps=[(1, 1, 0, 0, 0), (3, 0, 0, 0, 0)], grow=GROW * 3 / 2)], "four stages")
    assert 5.2 < float(tail) < 5.3


def test_inverse_fold_schedule_walk(emu):
    """Every inverse schedule, with the bound carried across steps and launches by the walk itself: a second launch that assumed a
    smaller entry bound than the first one leaves, or a limit above 8 q, fails here.  The product's inverse enters from 0.6 q."""
    for logn in range(1, 21):
        for form in (0, 1, 2):
            passes = _schedule(emu, form, logn, 1)
            if passes is None:
                continue
            top = _walk_inverse(emu, passes, None, (logn, form))
            assert top <= 8
            if form == 0 and logn in (3, 4, 12, 16, 20):
                assert top == 8                    # a first step of three stages or more: canonical words reach the limit, 1, 2, 4, 8
        mid = _schedule(emu, 3, logn, 1)
        second = _schedule(emu, 0, logn, 1)
        _walk_inverse(emu, [dict(mid[0], in_mode=1)] + (second[1:] if len(second) == 2 else []), Fr(6, 10) + SLACK, (logn, 3))


# ------------------------------------------------------------------ the emulation on the designed vectors
def _emu_one(emu, L, vec, inverse, form):
    got = _run(emu, vec[None, None, :], L.logn, inverse, [L.q], L.rp[None, :], 0, fused_dist=FORMS[form])[0, 0]
    return got, emu.emu_max_ratio(), emu.emu_max_pair()


def _check(emu, L, vec, inverse, form, reach, pair, what):
    emu.emu_max_pair.restype = C.c_double
    want = O.nwt_inverse(vec, L.q, L.rp) if inverse else O.nwt_forward(vec, L.q, L.rp)
    got, mx, mp = _emu_one(emu, L, vec, inverse, form)
    assert (got == want).all(), what
    assert mx < 8.0 and mp <= 8.0, (what, mx, mp)
    assert mx >= reach - 1e-12, (what, mx, reach)
    if inverse and pair is not None:
        assert mp >= pair - 1e-12, (what, mp, pair)
    return mx, mp


@pytest.mark.parametrize("logn", EMU_SIZES)
@pytest.mark.parametrize("bits", [50, 30])
def test_emulation_forward_ladder(emu, limbs, logn, bits):
    L = limbs(logn, bits)
    for form in _forms(logn, 0):
        for s0, K, canonical in W.forward_stretches(logn, canonical_at=(8,) if form == "packed" else ()):
            vec, _, reach, _ = W.forward_ladder(L, s0, K, canonical)
            _check(emu, L, vec, 0, form, reach, None, ("ladder", logn, bits, form, s0, K))


@pytest.mark.parametrize("logn", EMU_SIZES)
@pytest.mark.parametrize("bits", [50, 30])
def test_emulation_pulses(emu, limbs, logn, bits):
    L = limbs(logn, bits)
    for t in range(logn):
        vi, ri, pi = W.inverse_pulse(L, t)
        vf, rf = W.forward_pulse(L, t)
        for form in _forms(logn, 1):
            ri, pi = W.inverse_pulse_reach(L, t, KIND[form])       # what the model vouches for under this form's schedule
            _check(emu, L, vi, 1, form, ri, pi, ("inverse pulse", logn, bits, form, t))
        for form in _forms(logn, 0):
            _check(emu, L, vf, 0, form, rf, None, ("forward pulse", logn, bits, form, t))


@pytest.mark.parametrize("logn", EMU_SIZES)
@pytest.mark.parametrize("bits", [50, 30])
def test_emulation_soak_patterns(emu, limbs, logn, bits):
    L = limbs(logn, bits)
    for name, vec, rf, ri, pi in W.soak_patterns(L):
        for form in _forms(logn, 0):
            _check(emu, L, vec, 0, form, rf, None, (name, "forward", logn, bits, form))
        for form in _forms(logn, 1):
            if name == "all_qm1":
                ri, pi = W.all_qm1_inverse_reach(L, KIND[form])
            _check(emu, L, vec, 1, form, ri, pi, (name, "inverse", logn, bits, form))
