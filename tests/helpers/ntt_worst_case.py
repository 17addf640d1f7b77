"""Inputs that drive the FP64 transform's lazy range towards its bound, designed from outside: Python integers, exact fractions and
the oracle only -- nothing here imports the emulation or the library.

The FP64 path keeps residues as exact integers in doubles, in a signed lazy range that a fold schedule holds below 8 q < 2^53
(DESIGN.md "lazy FP64 ranges").  Every family below is one limb of N = 2^logn words together with the reach its model predicts for
the register it dictates, in units of q:

  ladder         forward: one register climbs by ~q/2 at every stage of a stretch between two folds
  inverse pulse  every word is congruent to one c ~ q/2 after t inverse stages
  forward pulse  the same after t forward stages
  soak           all q - 1, alternating blocks of every period, q/2, spikes (the patterns of tests/tools/soak.py, fixed seeds)

Model of the arithmetic (modarith.hpp ArithF64): every rounding is float(Fraction), which CPython rounds correctly, and rint is
round() on a float (ties to even), so model_mulmod / model_reduce give the very integer the kernel's register holds.
"""
from fractions import Fraction as Fr

import numpy as np

from oracle import cport as O


# ------------------------------------------------------------------ tables
def prime_below(bits: int, logn: int) -> int:
    """Largest prime below 2^bits that is 1 mod 2N."""
    return O.gen_primes(max(1 << logn, 2), bits, 1)[-1]


class Limb:
    """One modulus with the oracle's tables: rp[2^s + block] is stage s's factor, rp_inv its inverse."""

    def __init__(self, logn: int, bits: int):
        self.logn, self.N, self.bits = logn, 1 << logn, bits
        self.q = prime_below(bits, logn)
        self.psi = O.min_primitive_root(self.q, 2 << logn)
        self.rp = O.root_powers(self.q, logn, self.psi)
        self.rp_inv = O.root_powers(self.q, logn, pow(self.psi, -1, self.q))
        self.half = (self.q + 1) // 2          # 2^-1 mod q


def undo_forward_stage(L: Limb, a, s: int):
    """The state before forward stage s, from the state after it."""
    return O.modmul(O.nwt_inverse_stage(a, s, L.q, L.rp_inv), np.full(L.N, L.half, dtype=np.uint64), L.q)


def undo_inverse_stage(L: Limb, a, s: int):
    """The state before the inverse step of stage s (X + Y, (X - Y) S^-1), from the state after it."""
    return O.modmul(O.nwt_forward_stage(a, s, L.q, L.rp), np.full(L.N, L.half, dtype=np.uint64), L.q)


# ------------------------------------------------------------------ exact model of ArithF64
def _fl(x) -> Fr:
    return Fr(float(x))


def model_mulmod(a: int, w: int, q: int) -> int:
    """ArithF64::mulmod(a, encode(w, q)): h = a*w rounded, k = rint(a * (w/q)), l = fma(a, w, -h), (fma(-k, q, h)) + l."""
    wp = _fl(Fr(w, q))
    h = _fl(a * w)
    k = round(float(a * wp))
    low = _fl(a * w - h)
    r = _fl(h - k * q)
    out = _fl(r + low)
    assert out.denominator == 1
    return int(out)


def model_reduce(x: int, q: int) -> int:
    """ArithF64::reduce: x - q * rint(x * (1/q))."""
    k = round(float(x * _fl(Fr(1, q))))
    out = _fl(x - k * q)
    assert out.denominator == 1
    return int(out)


def centred(x: int, q: int) -> int:
    x %= q
    return x - q if 2 * x > q else x


def tie_margin(q: int) -> int:
    """Distance from q/2 beyond which reduce() of ANY lazy value below 8 q lands on the centred representative: the quotient
    estimate x * (1/q) is off by at most 8 * 2^-52 * 2, so a residue whose fraction of q stays 2^-40 away from 1/2 cannot tie."""
    return (q >> 40) + 1


# ------------------------------------------------------------------ (a) forward ladder
def _ladder_positions(L: Limb, s0: int, K: int):
    """Blocks of 2^K points that interact during stages s0 .. s0+K-1: the index bits above the field (the block of stage s0) and
    below it (the column), each first, middle and last, so that tiles of rows and of columns all meet one."""
    nlow = L.logn - s0 - K
    ps = sorted({0, (1 << s0) >> 1, (1 << s0) - 1})
    lows = sorted({0, (1 << nlow) >> 1, (1 << nlow) - 1})
    return [(p, lo) for p in ps for lo in lows]


def forward_ladder(L: Limb, s0: int, K: int, canonical: bool):
    """Stretch of K stages from stage s0.  ``canonical``: the stretch starts from canonical words (s0 = 0, or a hand-over of canonical
    residues), otherwise right after a fold.  Register 0 of each block holds c0 and its partner at stage s0 + i is an untouched word
    w_i^-1 h_i, whose product comes out as +h_i ~ q/2: register 0 reaches c0 + sum h_i.  h_i is the candidate (q-1)/2 - j, j < 64,
    nearest q/2 whose modelled product is positive (next to the rounding tie of the quotient estimate the sign is the model's to
    tell: one h per stage, so that every stage can be given a candidate that lands on the same side).
    Returns (input vector, state before stage s0, predicted reach of register 0 in units of q -- the largest over the blocks --,
    [(p, lo, the integer register 0 of block (p, lo) reaches)])."""
    q, logn = L.q, L.logn
    assert 0 <= s0 and s0 + K <= logn and K >= 1
    c0 = q - 1 if canonical else (q - 1) // 2 - tie_margin(q)
    state = np.zeros(L.N, dtype=np.uint64)
    reach, tops = 0, []
    for p, lo in _ladder_positions(L, s0, K):
        base = (p << (logn - s0)) | lo
        state[base] = c0
        top = c0
        for i in range(K):
            w = int(L.rp[(1 << (s0 + i)) + (p << i)])
            winv = pow(w, -1, q)
            y = h = 0                             # (no candidate lands on the positive side: the stage adds nothing)
            for j in range(64):
                hj = (q - 1) // 2 - j
                yj = winv * hj % q
                reg = yj if canonical else centred(yj, q)
                if not canonical and abs(2 * abs(reg) - q) <= 2 * tie_margin(q):
                    continue                      # the fold before the stretch could land on either side: not dictated
                if model_mulmod(reg, w, q) == hj:
                    y, h = yj, hj
                    break
            state[base + ((1 << (K - 1 - i)) << (logn - s0 - K))] = y
            top += h
        reach = max(reach, top)
        tops.append((p, lo, top))
    vec = state
    for s in range(s0 - 1, -1, -1):
        vec = undo_forward_stage(L, vec, s)
    return vec, state, reach / q, tops


# ------------------------------------------------------------------ (b), (c) pulses
def pulse_residue(q: int) -> int:
    """c just below q/2, far enough from the tie that every fold of a word congruent to c gives +c."""
    return (q - 1) // 2 - tie_margin(q)


def inverse_pulse(L: Limb, t: int):
    """Input whose state after t inverse steps (unscaled, as the kernels run them: the N^-1 comes last) is c everywhere.  Before
    step t every register is congruent to c, so its magnitude is at least c and a pair sum at least 2 c, whatever representative
    the lazy arithmetic holds; a register the schedule folds there becomes +c exactly and the sums of such registers double.
    Returns (input vector, predicted reach, predicted pair sum)."""
    c = pulse_residue(L.q)
    vec = np.full(L.N, c * pow(L.half, t, L.q) % L.q, dtype=np.uint64)      # (the t halvings of undo_inverse_stage, taken first)
    for v in range(t - 1, -1, -1):               # executed step v undoes forward stage logn - 1 - v
        vec = O.nwt_forward_stage(vec, L.logn - 1 - v, L.q, L.rp)
    return vec, c / L.q, 2 * c / L.q


def forward_pulse(L: Limb, t: int):
    """Input whose state after t forward stages is c everywhere.  Returns (input vector, predicted reach)."""
    c = pulse_residue(L.q)
    vec = np.full(L.N, c * pow(L.half, t, L.q) % L.q, dtype=np.uint64)
    for s in range(t - 1, -1, -1):
        vec = O.nwt_inverse_stage(vec, s, L.q, L.rp_inv)
    return vec, c / L.q


# ------------------------------------------------------------------ (d) soak patterns
def soak_patterns(L: Limb, seed: int = 12345):
    """[(name, vector, forward reach, inverse reach, inverse pair sum)].  All q - 1 doubles on the inverse's sum branch from canonical
    words: after two steps (every schedule allows two from canonical input) 4 (q - 1)."""
    q, N, logn = L.q, L.N, L.logn
    rng = np.random.default_rng(seed + logn)
    top = (q - 1) / q
    # (the last step multiplies N^-1 in, so its outputs are products: the sums double over min(logn - 1, 2) steps, the pairs over one more)
    out = [("all_qm1", np.full(N, q - 1, dtype=np.uint64), top, (1 << min(logn - 1, 2)) * top, (1 << min(logn, 2)) * top)]
    for lg in range(logn):
        v = np.where((np.arange(N) >> lg) % 2 == 0, 0, q - 1).astype(np.uint64)
        out.append((f"alt{lg}", v, top, top, top))
    out.append(("half", np.full(N, q // 2, dtype=np.uint64), (q // 2) / q, (q // 2) / q, 2 * (q // 2) / q))
    v = np.zeros(N, dtype=np.uint64)
    v[rng.integers(0, N, size=max(1, N // 64))] = q - 1
    out.append(("spikes", v, top, top, top))
    out.append(("near_q", rng.integers(q - min(q, 1000), q, N, dtype=np.uint64), (q - 1000) / q, (q - 1000) / q, 2 * (q - 1000) / q))
    return out


# ------------------------------------------------------------------ the schedule the families are aimed at
FWD_FIRST, FWD_NEXT = 5, 6       # the documented forward fold stages 5, 11, 17: restated here, not imported


def forward_stretches(logn: int, canonical_at=()):
    """[(s0, K, canonical)]: the runs of stages between folds; ``canonical_at``: stages before which the form hands canonical
    residues over (the packed hand-off)."""
    cuts = sorted({0} | {s for s in range(FWD_FIRST, logn, FWD_NEXT)} | set(canonical_at))
    out = []
    for i, s0 in enumerate(cuts):
        end = cuts[i + 1] if i + 1 < len(cuts) else logn
        if end > s0:
            out.append((s0, end - s0, s0 == 0 or s0 in canonical_at))
    return out


# ------------------------------------------------------------------ the inverse schedule, restated, and what a pulse does under it
# Restated from the documented plan (DESIGN.md section 3 "lazy ranges", ntt_plan.hpp's table of register steps): nothing is imported.
# tests/test_ntt_worst_case.py holds this restatement against what the templates produce.
PLAN_STEPS = {  # logn: (column steps, row steps), zeros dropped
    1: ((), (1,)), 2: ((), (2,)), 3: ((), (3,)), 4: ((), (4,)), 5: ((), (3, 2)), 6: ((), (3, 3)), 7: ((), (4, 3)), 8: ((), (4, 4)),
    9: ((), (3, 3, 3)), 10: ((), (4, 3, 3)), 11: ((), (4, 4, 3)), 12: ((), (4, 4, 4)), 13: ((3, 2), (4, 4)), 14: ((3, 3), (4, 4)),
    15: ((4, 3), (4, 4)), 16: ((4, 4), (4, 4)), 17: ((4, 4), (3, 3, 3)), 18: ((4, 4), (4, 3, 3)), 19: ((4, 4), (4, 4, 3)),
    20: ((4, 4), (4, 4, 4))}
RESIDENT_STEPS = {13: (5, 4, 4), 14: (5, 5, 4)}
INV_FIRST, INV_NEXT = 2, 3        # the uniform schedule of the fused and resident forms: every register before executed stage 2, 5, 8, ...
LIMIT8, EXIT8 = 64, 16            # per-register plan: fold where a pair's bound would pass 8 q; hand over at most 2 q


def inv_lazy_plan(K: int, in8: int, exit8: int, fold_last: bool):
    """The per-register plan of K inverse stages: bounds in 1/1024 q rounded up, a fold leaves 513, a product 513 + sum/4.
    Returns (before[K] register masks, at_exit mask, out8)."""
    R = 1 << K
    b = [in8 * 128] * R
    limit, folded = LIMIT8 * 128, 513
    before = []
    for v in range(K):
        u = K - 1 - v
        half = R >> (u + 1)
        m = 0
        for blk in range(1 << u):
            for j in range(half):
                i0 = blk * 2 * half + j
                i1 = i0 + half
                if b[i0] + b[i1] > limit:
                    big = i0 if b[i0] >= b[i1] else i1
                    b[big] = folded
                    m |= 1 << big
                    if b[i0] + b[i1] > limit:
                        other = i1 if big == i0 else i0
                        b[other] = folded
                        m |= 1 << other
                ssum = b[i0] + b[i1]
                prod = 513 + (ssum + 3) // 4
                b[i0] = prod if (fold_last and u == 0) else ssum
                b[i1] = prod
        before.append(m)
    at_exit = 0
    for r in range(R):
        if b[r] > exit8 * 128:
            b[r] = folded
            at_exit |= 1 << r
    return before, at_exit, (max(b) + 127) // 128


def inverse_schedule(logn: int, form: str):
    """[(first executed stage, K, before[K], at_exit, scaled last stage?)] in execution order.  form "plan": the two-launch /
    single-pass default (per-register plan); "mask": the fused launch; "resident": the LDS-resident pass."""
    col, row = PLAN_STEPS[logn]
    if form == "resident":
        col, row = (), RESIDENT_STEPS[logn]
    out, g, in8 = [], 0, 8
    for steps, last_pass in ((row, not col), (col, True)):
        for e, K in enumerate(reversed(steps)):
            last = last_pass and e == len(steps) - 1           # the step that ends with forward stage 0 and writes canonical words
            if form == "plan":
                before, at_exit, in8_next = inv_lazy_plan(K, in8, LIMIT8 if last else EXIT8, last)
                in8 = in8_next
            else:
                full = (1 << (1 << K)) - 1
                before = [full if (g + v >= INV_FIRST and (g + v - INV_FIRST) % INV_NEXT == 0) else 0 for v in range(K)]
                at_exit = 0
            out.append((g, K, before, at_exit, last))
            g += K
    assert g == logn
    return out


def _run_step(q, K, before, scaled, v0, val, res):
    """Registers of one thread from local stage v0 to the step's end.  val[r]: the exact lazy integer where the model knows it, else
    None; res[r]: its residue where known.  A fold makes a register of known residue known again (away from the tie); a sum of known
    registers is known; a product is known only where the difference is exactly 0.  Returns (largest known |value|, largest known
    pair sum), as integers."""
    R = 1 << K
    top = max([abs(x) for x in val if x is not None] + [0])
    pair = 0
    for v in range(v0, K):
        u = K - 1 - v
        half = R >> (u + 1)
        if v > v0:                                            # (stage v0's folds are the caller's starting point)
            for r in range(R):
                if (before[v] >> r) & 1:
                    if val[r] is not None:
                        val[r] = model_reduce(val[r], q)
                    elif res[r] is not None and abs(2 * (res[r] % q) - q) > 2 * tie_margin(q):
                        val[r] = centred(res[r], q)
        for blk in range(1 << u):
            for j in range(half):
                i0 = blk * 2 * half + j
                i1 = i0 + half
                x, y, rx, ry = val[i0], val[i1], res[i0], res[i1]
                known = x is not None and y is not None
                if known:
                    pair = max(pair, abs(x) + abs(y))
                same = rx is not None and ry is not None and (rx - ry) % q == 0
                res[i1] = 0 if same else None
                val[i1] = 0 if (known and x == y) else None
                if scaled and u == 0:
                    res[i0], val[i0] = None, None             # (s N^-1: a product)
                else:
                    res[i0] = (rx + ry) % q if rx is not None and ry is not None else None
                    val[i0] = x + y if known else None
                for z in (val[i0], val[i1]):
                    if z is not None:
                        top = max(top, abs(z))
    return top, pair


def inverse_pulse_reach(L: Limb, t: int, form: str):
    """What the model knows of the pulse at executed stage t under ``form``'s schedule: before stage t every register is congruent
    to c (magnitude at least c, pair sum at least 2 c, whatever the representative); the registers the schedule folds there -- or
    all of them at t = 0, canonical words -- hold +c exactly, and from there the sum branch carries c, 2 c, 4 c ... until the
    schedule folds it or the step ends.  Returns (reach, pair sum) in units of q for the register step that holds stage t."""
    q, c = L.q, pulse_residue(L.q)
    for g, K, before, at_exit, scaled in inverse_schedule(L.logn, form):
        if g <= t < g + K:
            R, v0 = 1 << K, t - g
            exact = (1 << R) - 1 if t == 0 else before[v0]
            val = [c if (exact >> r) & 1 else None for r in range(R)]
            top, pair = _run_step(q, K, before, scaled, v0, val, [c] * R)
            return max(top, c) / q, max(pair, 2 * c) / q
    raise AssertionError(t)


def all_qm1_inverse_reach(L: Limb, form: str):
    """All q - 1 through the first register step: q - 1, 2 (q - 1), 4 (q - 1) ... on the sum branch, folds as scheduled."""
    q = L.q
    g, K, before, at_exit, scaled = inverse_schedule(L.logn, form)[0]
    val, res = [q - 1] * (1 << K), [q - 1] * (1 << K)
    for r in range(1 << K):
        assert not (before[0] >> r) & 1
    top, pair = _run_step(q, K, before, scaled, 0, val, res)
    return top / q, pair / q
