"""Inputs designed for the natural-order transform's own network, from outside: Python integers and the oracle only -- nothing here
imports the emulation or the library.

The natural-order route (ntt_kernels.hip launch_gs_t: fhe_ntt_cyclic, the four-step calls) is the inverse-structured network of
tests/helpers/ntt_worst_case.py run on BIT-REVERSED input with a cyclic table in the inverse slot:

  table     tw[2^s + bitrev(k, s)] = (g^((q-1)/2^(s+1)))^k, tw[0] = 1 (host_math.hpp cyclic_table, restated here)
  network   bit-reverse, then (X, Y) -> (X + Y, (X - Y) tw[2^s + block]) for s = logn-1 .. 0, then times the scale
  forward   g, scale 1;  inverse   g^-1 (g^(q-2), motivation/bsgs.py), scale n^-1 folded into the last stage

A vector solved backwards through the NEGACYCLIC tables steers nothing here; every family below is built for this table, given in
natural order, and comes with the reach its model predicts in units of q.  The fold schedule of the route is the per-register plan
of the negacyclic inverse ("plan" in ntt_worst_case.py: same register steps, entry bound q, N^-1 -- here the scale -- folded into the
last stage); tests/test_gs_worst_case.py holds that statement against what the templates of this route produce."""
import numpy as np

from oracle import cport as O
from helpers import ntt_worst_case as W

GS_FORM = "plan"                 # the schedule this route gets: GsPasses::First / Second are Passes<A, LOGN, true, GEO>'s plan family


def _is_prime(n: int) -> bool:
    if n < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % p == 0:
            return n == p
    d, r = n - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):       # deterministic below 3.3e24
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(r - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def largest_prime(bits: int, N: int) -> int:
    """Largest prime below 2^bits that is 1 mod N (the cyclic transform needs no 2N-th root)."""
    p = ((1 << bits) - 2) // N * N + 1
    while not _is_prime(p):
        p -= N
    return p


def bitrev_perm(logn: int) -> np.ndarray:
    idx = np.arange(1 << logn, dtype=np.int64)
    out = np.zeros_like(idx)
    for b in range(logn):
        out |= ((idx >> b) & 1) << (logn - 1 - b)
    return out


def cyclic_table(q: int, logn: int, g: int) -> np.ndarray:
    tw = np.zeros(1 << logn, dtype=np.uint64)
    tw[0] = 1 % q
    for s in range(logn):
        w = pow(g, (q - 1) >> (s + 1), q)
        p, pw = 1 % q, []
        for _ in range(1 << s):
            pw.append(p)
            p = p * w % q
        tw[(1 << s) + bitrev_perm(s)] = pw
    return tw


class GsLimb:
    """One modulus of the natural-order route in one direction: tw is the table the network multiplies by, tw_inv its element-wise
    inverses, scale what the last stage folds in.  ``bits`` picks the largest prime below 2^bits that is 1 mod N, g the smallest
    quadratic non-residue (a root of every power-of-two order dividing q - 1)."""

    def __init__(self, logn: int, bits: int, inverse: bool = False, q: int = 0, g: int = 0):
        self.logn, self.N, self.bits, self.inverse = logn, 1 << logn, bits, inverse
        self.q = q or largest_prime(bits, self.N)
        assert (self.q - 1) % self.N == 0
        self.g = g or next(x for x in range(2, 1000) if pow(x, (self.q - 1) // 2, self.q) == self.q - 1)
        used = pow(self.g, self.q - 2, self.q) if inverse else self.g
        self.tw = cyclic_table(self.q, logn, used)
        self.tw_inv = cyclic_table(self.q, logn, pow(used, self.q - 2, self.q))
        self.scale = pow(self.N, self.q - 2, self.q) if inverse else 1
        self.half = (self.q + 1) // 2
        self.perm = bitrev_perm(logn)

    def oracle(self, vec):
        return (O.intt_cyclic if self.inverse else O.ntt_cyclic)(vec, self.q, self.g)


def stages(L: GsLimb, state, t: int):
    """``t`` executed stages of the network from ``state`` (network order, i.e. the input already bit-reversed)."""
    for v in range(t):
        state = O.nwt_inverse_stage(state, L.logn - 1 - v, L.q, L.tw)
    return state


def network(L: GsLimb, vec):
    """The whole staged transform of a natural-order vector: natural-order result, scaled."""
    out = stages(L, np.ascontiguousarray(np.asarray(vec, dtype=np.uint64)[L.perm]), L.logn)
    return O.modmul(out, np.full(L.N, L.scale, dtype=np.uint64), L.q)


def natural_pulse(L: GsLimb, t: int):
    """Natural-order input whose state after t executed stages is c = pulse_residue(q) everywhere: executed stage v is undone by the
    forward stage logn-1-v over the inverse table, times 2^-1.  Returns (vector, predicted reach, predicted pair sum): what
    ntt_worst_case.inverse_pulse_reach vouches for under this route's schedule."""
    c = W.pulse_residue(L.q)
    state = np.full(L.N, c * pow(L.half, t, L.q) % L.q, dtype=np.uint64)
    for v in range(t - 1, -1, -1):
        state = O.nwt_forward_stage(state, L.logn - 1 - v, L.q, L.tw_inv)
    reach, pair = W.inverse_pulse_reach(L, t, GS_FORM)
    return np.ascontiguousarray(state[L.perm]), reach, pair


def constant_reach(L: GsLimb, c0: int):
    """EXACT reach and pair sum of the constant vector c0 over the whole schedule.  The bit reversal leaves it alone; after v
    stages the words at multiples of 2^v hold the doubled sum and every other word is 0, so in each register step a thread holds 2^K
    equal registers or 2^K zeros, and one register's exact integer (W.model_reduce at the plan's folds) is the whole state."""
    q, x = L.q, c0
    top = pair = 0
    for g, K, before, at_exit, scaled in W.inverse_schedule(L.logn, GS_FORM):
        R = 1 << K
        val = [W.model_reduce(x, q) if (before[0] >> r) & 1 else x for r in range(R)]
        top = max(top, abs(x))
        t, p = W._run_step(q, K, before, scaled, 0, val, [x % q] * R)
        top, pair = max(top, t), max(pair, p)
        if scaled:
            break                                      # (the last stage leaves products below q: no new maximum)
        x = val[0]
        assert x is not None and all(v == 0 for v in val[1:])
        if at_exit & 1:
            x = W.model_reduce(x, q)
    return top / q, pair / q


def families(L: GsLimb, pulses=None, seed: int = 12345):
    """[(name, natural-order vector, predicted reach, predicted pair sum, exact?)].  exact: the model gives the tracker's figure itself,
    not a floor.  ``pulses``: the stages to build pulses for (default: every stage)."""
    q, N, logn = L.q, L.N, L.logn
    rng = np.random.default_rng(seed + logn + (1 << 20 if L.inverse else 0))
    top = (q - 1) / q
    out = []
    for t in (range(logn) if pulses is None else sorted(set(pulses))):
        v, reach, pair = natural_pulse(L, t)
        out.append((f"pulse{t}", v, reach, pair, False))
    out.append(("all_qm1", np.full(N, q - 1, dtype=np.uint64), *constant_reach(L, q - 1), True))
    out.append(("half", np.full(N, q // 2, dtype=np.uint64), *constant_reach(L, q // 2), True))
    for lg in range(logn):
        # blocks of 2^lg zeros and 2^lg words q - 1 in NETWORK order: period 2 is the first stage's own pairs (0, q - 1), longer periods
        # pair equal words for lg stages first
        pat = np.where((np.arange(N) >> lg) % 2 == 0, 0, q - 1).astype(np.uint64)
        out.append((f"alt{lg}", np.ascontiguousarray(pat[L.perm]), top, top, False))
    v = np.zeros(N, dtype=np.uint64)
    v[rng.integers(0, N, size=max(1, N // 64))] = q - 1
    out.append(("spikes", v, top, top, False))
    lo = q - min(q, 1000)
    out.append(("near_q", rng.integers(lo, q, N, dtype=np.uint64), lo / q, 2 * lo / q, False))
    return out


def random_vector(L: GsLimb, seed: int = 777):
    return np.random.default_rng(seed + L.logn).integers(0, L.q, L.N, dtype=np.uint64)
