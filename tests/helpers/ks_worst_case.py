"""Inputs that dictate the internals of the key switch, the rescale and the homomorphic multiply.

The composites are compared with the oracle bit for bit, but random limbs never reach the places where their kernels could be
wrong: the lazy accumulators of the inner product (FP64: |term| < 0.875 q, a fold after every eighth term, 8 q < 2^53; U64: a
128-bit sum of eight products), the borrow and carry edges of the mod-down's tail, the narrow window in which a coefficient
below one prime is not below its neighbour, and the largest mixed-radix digits of the conversions.  All of these can be set
from outside, because the NTT is a bijection and the switching key is a free input:

* an input limb is the oracle's forward transform of a chosen coefficient vector (edge_coefficients, digit_columns);
* the extended digit x_d[j][i] follows from c alone (extended_digits restates oracle/keyswitch_ref.py), the key word y_d[j][i]
  is free: x y mod q is any chosen residue (product_families, same_sign_block), and acc[h][j][i] = sum_d x_d y_d is any chosen
  word (solve_key_for_acc), so the special rows of acc are the transform of a chosen vector over the special base and the
  difference the tail sees is a chosen edge (tail_targets).

This file DESIGNS inputs and reports the magnitudes they reach.  It never forms an expected value: that is the oracle's part.
Python integers and numpy doubles only (the doubles restate the kernels' operation order as a design aid); the oracle's batch
primitives serve for the transforms and for batched modular powers.  No kernel and not the package is imported.
"""
import numpy as np

from oracle import cport as O

from . import bc_worst_case as W

U = np.uint64
# residues of x y next to q / 2, where the FP64 quotient estimate rint(x y / q) decides between k and k + 1
NEAR_HALF = ("half-", "half+", "half--", "half++")
FAMILIES = NEAR_HALF + ("q-1", "one", "zero", "ymax")


def family_target(name, q):
    """the residue x y mod q of a family (None for "ymax", which fixes y = q - 1 instead)"""
    return {"half-": (q - 1) // 2, "half+": (q + 1) // 2, "half--": (q - 1) // 2 - 1, "half++": (q + 1) // 2 + 1, "q-1": q - 1, "one": 1,
            "zero": 0, "ymax": None}[name]


def _tables(qs, logn):
    return np.stack([O.root_powers(int(q), logn) for q in qs])


def mul(a, b, q):
    """a b mod q word by word, arrays of one shape"""
    return O.modmul(np.ascontiguousarray(a, dtype=U).reshape(-1), np.ascontiguousarray(b, dtype=U).reshape(-1), int(q)).reshape(np.shape(a))


def inverse_words(x, q):
    """x^(q-2) mod q word by word (0 stays 0), by square and multiply over the whole array"""
    x = np.ascontiguousarray(x, dtype=U)
    out, base, e = np.ones_like(x), x.copy(), int(q) - 2
    while e:
        if e & 1:
            out = mul(out, base, q)
        base = mul(base, base, q)
        e >>= 1
    return out


def extended_digits(c, qs, L, K, dnum, logn, rps=None):
    """[dnum][M][N]: the words x_d the inner product multiplies with the key (oracle/keyswitch_ref.py keyswitch_ref lines 44-52: INTT of
    the input limbs, exact conversion of each digit to every other limb, forward transform, the digit's own limbs copied)"""
    M, N = L + K, 1 << logn
    alpha = -(-L // dnum)
    qs = [int(q) for q in qs]
    rps = _tables(qs, logn) if rps is None else rps
    c = np.asarray(c, dtype=U)
    coef = O.nwt_inverse_batch(c, qs[:L], rps[:L])
    x = np.zeros((dnum, M, N), dtype=U)
    for d in range(dnum):
        lo, hi = d * alpha, min(L, (d + 1) * alpha)
        other = [j for j in range(M) if j < lo or j >= hi]
        conv = O.baseconv_exact(coef[lo:hi], qs[lo:hi], [qs[j] for j in other])
        x[d, other] = O.nwt_forward_batch(conv, [qs[j] for j in other], rps[other])
        x[d, lo:hi] = c[lo:hi]
    return x


def edge_values(q, others):
    """the coefficients below q at which a reduction modulo q, modulo a neighbour or a conversion to and from doubles can go wrong"""
    v = [0, 1, q - 1, (q - 1) // 2, (q + 1) // 2]
    for p in others:
        v += [p - 1, p, p + 1, q - p, 2 * p, q // p * p - 1, q // p * p, q // p * p + 1]
    if q >= 1 << 50:
        v += [(1 << 50) - 1, 1 << 50, (1 << 52) - 1, 1 << 52, 1 << 53]          # the edges of from_canonical / to_u64
    out = []
    for e in v:
        if 0 <= e < q and e not in out:
            out.append(e)
    return out


def edge_coefficients(q, others, N, seed=0):
    """length-N vector of [0, q): edge_values(q, others) first (as many as fit), then random fill"""
    q = int(q)
    rng = np.random.default_rng([seed, q % (1 << 31)])
    out = rng.integers(0, q, N, dtype=U)
    e = edge_values(q, [int(p) for p in others])[:N]
    out[:len(e)] = np.array(e, dtype=U)
    return out


def digit_columns(base, targets, N, seed=0):
    """[len(base)][N] residue columns over ``base`` whose mixed-radix digits are bc_worst_case.worst_columns(base, targets) (the digits
    and split FP64 sums of the conversion kernels at their largest magnitude), then random fill; also the names of the columns set"""
    base, targets = [int(p) for p in base], [int(q) for q in targets]
    rng = np.random.default_rng([seed, len(base), N])
    out = np.stack([rng.integers(0, p, N, dtype=U) for p in base])
    cols = W.worst_columns(base, targets)[:N]
    for i, (_, digs) in enumerate(cols):
        out[:, i] = np.array(W.residues_from_digits(base, digs), dtype=U)
    return out, [name for name, _ in cols]


def f64_terms(x, y, q):
    """Design aid: the FP64 path's term h - k q + l of every word pair, as the signed integer it is (KsMacF64's operation order in
    numpy doubles: k = rint(x * (y * (1 / q))); the value x y - k q is formed in 64-bit wrap-around integers, exact below 2^63)."""
    x, y = np.asarray(x, dtype=U), np.asarray(y, dtype=U)
    ninv = 1.0 / float(q)
    k = np.rint(x.astype(np.float64) * (y.astype(np.float64) * ninv))
    return (x * y - k.astype(np.int64).astype(U) * U(q)).astype(np.int64)


def product_families(x, q, path, xinv=None):
    """x: words != 0 of [0, q).  -> {family: y} with x y mod q = family_target(family, q) (and y = q - 1 for "ymax"); on the FP64 path
    ("f64") also {family: signed term} from f64_terms.  ``xinv`` = inverse_words(x, q) when the caller already has it."""
    q = int(q)
    x = np.asarray(x, dtype=U)
    assert (x != 0).all() and (x < U(q)).all()
    xinv = inverse_words(x, q) if xinv is None else xinv
    ys, terms = {}, {}
    for name in FAMILIES:
        t = family_target(name, q)
        ys[name] = np.full(x.shape, q - 1, dtype=U) if t is None else mul(xinv, np.full(x.shape, t, dtype=U), q)
        if path == "f64":
            terms[name] = f64_terms(x, ys[name], q)
    return (ys, terms) if path == "f64" else ys


def running_sums(x, y, q, path, fold=8):
    """Reach of the lazy accumulator over the terms x[t] y[t] (t = axis 0), from exact integers: (largest value before a fold, largest
    value before the final reduction).  FP64: |s| of the signed terms, the fold s -= rint(s / q) q as ArithF64::reduce estimates it;
    U64: the 128-bit sum, the fold s %= q.  Python integers for U64 (keep the arrays small), 64-bit integers for FP64."""
    T = x.shape[0]
    if path == "f64":
        ninv, s, before = 1.0 / float(q), np.zeros(x.shape[1:], dtype=np.int64), 0
        for t in range(T):
            s = s + f64_terms(x[t], y[t], q)
            if t % fold == fold - 1:
                before = max(before, int(np.abs(s).max()))
                s = s - np.rint(s.astype(np.float64) * ninv).astype(np.int64) * np.int64(q)
        return before, int(np.abs(s).max())
    s, before = [0] * x[0].size, 0
    xs, ys = x.reshape(T, -1), y.reshape(T, -1)
    for t in range(T):
        s = [a + int(b) * int(c) for a, b, c in zip(s, xs[t], ys[t])]
        if t % fold == fold - 1:
            before = max(before, max(s))
            s = [a % q for a in s]
    return before, max(s)


def same_sign_block(x, q, path, xinv=None):
    """x: [T][...] words != 0.  -> (y [T][...], reach): key words from the near-half families such that, per slot, the eight terms of a
    fold block all have one sign (the largest magnitude of that sign the families offer: up to (q + 3) / 2 where the quotient estimate
    rounds to the far side; even slots take +, odd slots -, in every block, so that a sum which missed a fold would keep growing).
    U64 has no signs: y = q - 1 everywhere, the largest products.  reach = running_sums(x, y, q, path)."""
    q = int(q)
    x = np.asarray(x, dtype=U)
    if path != "f64":
        y = np.full(x.shape, q - 1, dtype=U)
        return y, running_sums(x, y, q, path) if x[0].size <= 4096 else None
    slot = np.arange(x[0].size, dtype=np.int64).reshape(x[0].shape)
    want = np.broadcast_to(np.where(slot % 2 == 0, 1, -1), x.shape)
    xinv = inverse_words(x, q) if xinv is None else xinv
    best, best_y = np.full(x.shape, -1, dtype=np.int64), np.zeros_like(x)
    for name in NEAR_HALF:
        yc = mul(xinv, np.full(x.shape, family_target(name, q), dtype=U), q)
        score = f64_terms(x, yc, q) * want          # > 0 on the wanted side
        take = score > best
        best, best_y = np.where(take, score, best), np.where(take, yc, best_y)
    # about one word in sixteen has all four estimates rounding to the other side: there a residue a quarter of q inside the
    # wanted side, whose sign no rounding can change
    quarter = np.where(want > 0, U(q // 4), U(q - q // 4))
    y = np.where(best > 0, best_y, mul(xinv, quarter, q))
    return y, running_sums(x, y, q, path)


def solve_key_for_acc(x, y, acc_target, qs):
    """x: [dnum][M][N]; y: [dnum][2][M][N] (any key); acc_target: [2][M][N].  -> (key, undictated): ``key`` is y with one digit's word
    per (half, row, slot) solved so that sum_d x_d y_d = acc_target mod q_row -- the first digit whose x_d != 0 there --, ``undictated``
    the count of words where every x_d is 0 (left as they are)."""
    dnum, M = x.shape[0], x.shape[1]
    key, undictated = np.array(y, dtype=U, copy=True), 0
    for j in range(M):
        q = int(qs[j])
        nz = x[:, j] != 0
        first = np.argmax(nz, axis=0)                       # per slot: the digit that is solved
        undictated += 2 * int((~nz.any(axis=0)).sum())
        for d in np.unique(first):
            sel = (first == d) & nz.any(axis=0)
            if not sel.any():
                continue
            xinv = inverse_words(x[d, j, sel], q)
            for h in range(2):
                rest = np.zeros(int(sel.sum()), dtype=U)
                for e in range(dnum):
                    if e != d:
                        rest = (rest + mul(x[e, j, sel], key[e, h, j, sel], q)) % U(q)
                need = (np.asarray(acc_target[h][j], dtype=U)[sel] + (U(q) - rest)) % U(q)
                key[d, h, j, sel] = mul(need, xinv, q)
    return key, undictated


TAIL_EDGES = ("equal", "borrow", "one", "half", "carry")


def tail_targets(cn, q, add=False, pinv=1, seed=0):
    """cn: [N] words the tail subtracts (NTT(conv)_j).  -> (acc_j, addend or None).  acc_j - cn_j mod q cycles through 0 (acc_j == cn_j),
    q - 1 (acc_j == cn_j - 1: the borrow by one), 1, (q - 1) / 2 and -pinv^-1 (the scaled word v = diff pinv is then q - 1) on the
    first 40 slots and every third slot after them; the rest is random.  With ``add`` the addend makes v + add equal q - 1, q, and
    2 q - 2 where v = q - 1 (else 2 q - 2 - (q - 1 - v), the largest sum that v allows), in turn."""
    q, N = int(q), len(cn)
    cn = np.asarray(cn, dtype=U)
    rng = np.random.default_rng([seed, q % (1 << 31), N])
    diff = rng.integers(0, q, N, dtype=U)
    edges = [0, q - 1, 1, (q - 1) // 2, (q - pow(int(pinv), -1, q)) % q]
    idx = np.arange(N)
    hit = (idx < 40) | (idx % 3 == 0)
    rank = np.cumsum(hit) - 1                               # the edges in turn over the slots that carry one
    diff[hit] = np.array(edges, dtype=U)[rank[hit] % 5]
    acc = (cn + diff) % U(q)
    if not add:
        return acc, None
    v = mul(diff, np.full(N, int(pinv), dtype=U), q)
    sums = np.array([q - 1, q, 2 * q - 2], dtype=U)[(rank // 5) % 3]
    addend = np.where(sums >= v, sums - v, U(0))
    addend = np.minimum(addend, U(q - 1))          # v + add = 2 q - 2 needs v = q - 1; elsewhere the largest addend
    return acc, addend


def tail_diff(acc, cn, q):
    """(acc - cn) mod q as the oracle's tail forms it (keyswitch_ref line 77)"""
    return (np.asarray(acc, dtype=U) + (U(q) - np.asarray(cn, dtype=U))) % U(q)
