"""Inputs on which the integer path (modarith.hpp ArithU64: Harvey butterflies with Shoup quotients, lazy words in [0, 4q) forward and
[0, 2q) inverse, one barrett128 step for a product of lazy words, a two-step canonical()) meets EQUALITY in its comparisons, designed
from outside: Python integers, tests/helpers/number_theory.py and the oracle only -- nothing here imports the emulation or the library.

Every decision on that path is ``x >= 2q`` or ``x >= q``.  A random 61-bit word meets equality with probability 2^-61, so random
vectors cannot tell ``>=`` from ``>``; a transform whose exact result VANISHES meets it all the time, because a vanishing word is held
as the lazy word 0, q, 2q or 3q.  The families:

  transform   the oracle's inverse image of a spectrum that is all zero, one nonzero slot (first, middle, last), zero on the first
              half, zero on the odd slots; and the first two with every third word lifted to another 64-bit word of its residue class
              (w + q, w + 2q, the largest below 2^64), which the ABI reduces first.  The inverse families mirror them.  Forward
              only, from 2^3 on: fold_tail, which brings the lazy pair (2q, 0) to the last stage (see fold_tail).
  product     (a, b, c): spectra with disjoint supports (c = 0), supports that meet in one slot, and b = x^j against an a with zeros
              at known places (c holds q - a_i, a_i and exact zeros)
  natural     the same supports under the oracle's cyclic definition, for fhe_ntt_cyclic and the four-step calls

and a model of ArithU64 in Python integers (class Model) run over a plain radix-2 network on the oracle's table, in which every
comparison is the real ``>=`` or, one site at a time, the mutant ``>``, and which counts the equalities it meets."""
from collections import Counter

import numpy as np

from helpers import number_theory as NT
from oracle import cport as O

M64 = (1 << 64) - 1
# one mutant per comparison site: the fold of bfly_fwd, the sum of bfly_inv, the two lines of canonical(), the two fix-ups of barrett128
SITES = ("fwd_fold", "inv_sum", "canon1", "canon2", "barrett1", "barrett2")
EQUALITIES = ("fold_eq", "sum_eq", "final_q", "final_2q", "final_3q", "barrett_q")


# ------------------------------------------------------------------ moduli and tables
def moduli(logn: int) -> list:
    """[largest, second largest prime below 2^61, smallest prime >= 2^50] that are 1 mod 2N: the top of the promised range twice and
    the lowest modulus that takes the integer path by size."""
    N = 1 << logn
    second, largest = NT.create_moduli(N, [61, 61])
    lowest = NT.first_prime_above((1 << 50) - 1, N)
    assert (1 << 50) <= lowest < second < largest < (1 << 61)
    return [largest, second, lowest]


class Limb:
    """One modulus with the oracle's table: rp[2^s + block] is stage s's factor."""

    def __init__(self, logn: int, q: int):
        self.logn, self.N, self.q = logn, 1 << logn, q
        self.psi = O.min_primitive_root(q, 2 << logn)
        self.rp = O.root_powers(q, logn, self.psi)


def limbs(logn: int) -> list:
    return [Limb(logn, q) for q in moduli(logn)]


# ------------------------------------------------------------------ supports
def supports(N: int):
    """[(name, mask of the slots that are NOT zero)]"""
    idx = np.arange(N)
    out = [("zero", np.zeros(N, dtype=bool))]
    for k in sorted({0, N // 2, N - 1}):
        out.append((f"slot_{k}", idx == k))
    out.append(("half_lo", idx >= N // 2))           # zero on the first half
    out.append(("odd", idx % 2 == 0))                # zero on the odd slots
    return out


def _sparse(rng, q: int, mask) -> np.ndarray:
    """random NONZERO words on the mask, exact zeros elsewhere"""
    return np.where(mask, rng.integers(1, q, mask.size, dtype=np.uint64), np.uint64(0)).astype(np.uint64)


def lift(vec, q: int) -> np.ndarray:
    """every third word replaced by another 64-bit word of its residue class: w + q, w + 2q, the largest below 2^64, in turn"""
    out = np.array(vec, dtype=np.uint64)
    assert int(out.max()) < q < (1 << 61)                # (so w + 2q stays below 2^64)
    Q = np.uint64(q)
    w = out[::3]
    turn = np.arange(w.size) % 3
    out[::3] = w + np.where(turn == 0, Q, np.where(turn == 1, Q + Q, (np.uint64(M64) - w) // Q * Q))
    assert (out % Q == np.asarray(vec, dtype=np.uint64)).all()
    return out


def transform_families(L: Limb, inverse: bool, seed: int = 2024, integer_path: bool = True):
    """[(name, input, expected output, mask)]: the expected output is zero exactly off the mask.  Forward: the input is the oracle's
    inverse image of the spectrum; inverse: the oracle's forward image of the coefficient vector.  ``integer_path`` False: a limb
    of the FP64 path riding along -- the same families, fold_tail's spectrum without the search for the lazy word 2q."""
    rng = np.random.default_rng(seed + 97 * L.logn + (1 if inverse else 0))
    out = []
    for name, mask in supports(L.N):
        want = _sparse(rng, L.q, mask)
        vec = (O.nwt_forward if inverse else O.nwt_inverse)(want, L.q, L.rp)
        out.append((name, vec, want, mask))
        if name == "zero" or name.startswith("slot_"):
            out.append(("lifted_" + name, lift(vec, L.q), want, mask))
    if not inverse and L.logn >= 3:
        vec, want = fold_tail(L, seed, search=integer_path)
        out.append(("fold_tail", vec, want, want != 0))
    return out


def fold_tail(L: Limb, seed: int = 2024, search: bool = True):
    """The family the forward fold's mutant needs.  An unfolded X = 2q only matters where the butterfly's product is exactly 0 in the
    LAST stage: then Y' = 2q - 0 + 2q = 4q, one q more than canonical() removes; anywhere else the next fold or canonical() absorbs it.
    A lazy word is exactly 0 only on the all-sums branch of an all-zero cone, so the pair is slots (0, 1): the odd coefficients are
    all zero (a spectrum with S[2i] = S[2i+1]), S[0] = S[1] = 0, and the even half's all-sums word before the last stage has to be
    the lazy word 2q rather than 0, q or 3q -- which the model decides: the first seed that gives it is taken."""
    q, N = L.q, L.N
    for k in range(256):
        rng = np.random.default_rng(seed + 7919 * L.logn + k)
        pairs = rng.integers(1, q, N // 2, dtype=np.uint64)
        pairs[0] = 0
        want = np.repeat(pairs, 2)
        vec = O.nwt_inverse(want, q, L.rp)
        assert not vec[1::2].any()
        if not search:
            return vec, want
        state = lazy_forward_np(L, vec, L.logn - 1)
        if int(state[0]) == 2 * q and int(state[1]) == 0:
            return vec, want
    raise AssertionError("no seed puts the lazy word 2q next to an exact 0 before the last stage")


def _mulhi(a, b):
    m, s = np.uint64(0xFFFFFFFF), np.uint64(32)
    a0, a1, b0, b1 = a & m, a >> s, b & m, b >> s
    mid1 = a1 * b0 + ((a0 * b0) >> s)
    mid2 = a0 * b1 + (mid1 & m)
    return a1 * b1 + (mid1 >> s) + (mid2 >> s)


def lazy_forward_np(L: Limb, vec, stages: int) -> np.ndarray:
    """The lazy words of Model(L).forward_lazy (no mutant, canonical input) after ``stages`` stages, in wrapping uint64 arithmetic:
    the search of fold_tail at sizes where the integer model takes seconds.  tests/test_harvey_cases.py holds it against the model."""
    q, two_q = np.uint64(L.q), np.uint64(2 * L.q)
    shoup = np.array([(int(w) << 64) // L.q for w in L.rp], dtype=np.uint64)
    a = np.array(vec, dtype=np.uint64)
    for s in range(stages):
        m, t = 1 << s, L.N >> (s + 1)
        v3 = a.reshape(m, 2, t)
        X, Y = v3[:, 0, :], v3[:, 1, :]
        w, wq = L.rp[m:2 * m, None], shoup[m:2 * m, None]
        x = np.where(X >= two_q, X - two_q, X)
        v = Y * w - _mulhi(Y, wq) * q
        a = np.stack([x + v, x - v + two_q], axis=1).reshape(L.N)
    return a


def random_vectors(L: Limb, count: int = 8, seed: int = 31337):
    """canonical random vectors with fixed seeds: what every other test of this path feeds it"""
    return [np.random.default_rng(seed + 1000 * L.logn + i).integers(0, L.q, L.N, dtype=np.uint64) for i in range(count)]


def _monomial_product(a, j: int, q: int) -> np.ndarray:
    """a x^j mod (x^N + 1, q), by its definition"""
    c = np.roll(np.asarray(a, dtype=np.uint64), j)       # c[(i + j) mod N] = a[i] ...
    c[:j] = (np.uint64(q) - c[:j]) % np.uint64(q)        # ... negated where i + j >= N
    return c


def product_families(L: Limb, seed: int = 4242):
    """[(name, a, b, expected c = a b mod (x^N + 1, q))]"""
    N, q = L.N, L.q
    rng = np.random.default_rng(seed + 97 * L.logn)
    idx = np.arange(N)
    out = []
    pairs = [("disjoint_halves", idx < N // 2, idx >= N // 2), ("disjoint_even_odd", idx % 2 == 0, idx % 2 == 1),
             ("meet_one_slot", idx <= N // 2, idx >= N // 2)]
    for name, ma, mb in pairs:
        A, B = _sparse(rng, q, ma), _sparse(rng, q, mb)
        assert int((ma & mb).sum()) == (1 if name == "meet_one_slot" else 0)
        c = O.nwt_inverse(O.modmul(A, B, q), q, L.rp)
        assert name == "meet_one_slot" or not c.any()
        out.append((name, O.nwt_inverse(A, q, L.rp), O.nwt_inverse(B, q, L.rp), c))
    for j in sorted({1, N // 2, N - 1}):
        a = _sparse(rng, q, idx % 4 != 1)              # zeros at 1, 5, 9, ...
        b = np.zeros(N, dtype=np.uint64)
        b[j] = 1
        out.append((f"monomial_{j}", a, b, _monomial_product(a, j, q)))
    return out


# ------------------------------------------------------------------ natural order
class CyclicLimb:
    """The cyclic transform's modulus: the largest prime below 2^61 that is 1 mod 2N (so 1 mod N), with the smallest quadratic
    non-residue as generator -- a root whose stage roots form the tower the natural-order launches and fhe_fourstep_create ask for."""

    def __init__(self, logn: int):
        self.logn, self.N = logn, 1 << logn
        self.q = moduli(logn)[0]
        self.g = next(x for x in range(2, 1000) if pow(x, (self.q - 1) // 2, self.q) == self.q - 1)
        self.w = pow(self.g, (self.q - 1) // self.N, self.q)        # the n-th root of the other convention
        assert pow(self.w, self.N // 2, self.q) == self.q - 1


def natural_families(Cy: CyclicLimb, inverse: bool, seed: int = 777):
    """[(name, natural-order input, expected natural-order output, mask)] under the oracle's cyclic definition"""
    rng = np.random.default_rng(seed + 97 * Cy.logn + (1 if inverse else 0))
    out = []
    for name, mask in supports(Cy.N):
        want = _sparse(rng, Cy.q, mask)
        vec = (O.ntt_cyclic if inverse else O.intt_cyclic)(want, Cy.q, Cy.g)
        out.append((name, vec, want, mask))
        if name == "zero" or name.startswith("slot_"):
            out.append(("lifted_" + name, lift(vec, Cy.q), want, mask))
    return out


def nthroot(vec, Cy: CyclicLimb, inverse: bool) -> np.ndarray:
    """the oracle's cyclic transform under the n-th root convention, root w = g^((q-1)/N)"""
    if not inverse:
        return O.ntt_nthroot(vec, Cy.w, Cy.q)
    a = np.ascontiguousarray(vec, dtype=np.uint64).copy()
    O.lib().orc_intt_cyclic_nthroot(a.ctypes.data_as(O.p64), a.size, Cy.w, Cy.q)
    return a


# ------------------------------------------------------------------ the model
class Model:
    """ArithU64 in Python integers over a plain radix-2 network on the oracle's table (forward: stages 0 .. logn-1; inverse: stages
    logn-1 .. 1 and the last one with N^-1 folded in, as the kernels run it).  ``mutant``: the sites whose ``>=`` is ``>``.
    events: fold_eq (X == 2q at the forward fold), sum_eq (X + Y == 2q at the inverse sum), final_q / final_2q / final_3q (the word
    on entry to canonical), shoup_hi (a Shoup product in [q, 2q)), barrett_q (barrett128 left exactly q before its first fix-up),
    range (an operand outside the documented range: >= 4q forward, >= 2q inverse)."""

    def __init__(self, L: Limb, mutant=()):
        self.L, self.q, self.two_q = L, L.q, 2 * L.q
        self.mutant = (mutant,) if isinstance(mutant, str) else tuple(mutant)
        assert all(s in SITES for s in self.mutant)
        q = L.q
        enc = lambda w: (w, (w << 64) // q)                           # ArithU64::encode
        self.fwd = [enc(int(w)) for w in L.rp]
        self.inv = [enc(pow(int(w), -1, q)) for w in L.rp]
        ninv = pow(L.N, -1, q)
        self.n = enc(ninv)
        self.wn = enc(ninv * self.inv[1][0] % q)    # inverse entry 0: N^-1 times the last stage's factor
        self.ratio = (1 << 128) // q
        self.events = Counter()

    def _ge(self, site, x, y):
        return x > y if site in self.mutant else x >= y

    def mulmod(self, a, t):
        r = (a * t[0] - ((a * t[1]) >> 64) * self.q) & M64
        assert r < self.two_q
        if r >= self.q:
            self.events["shoup_hi"] += 1
        return r

    def bfly_fwd(self, X, Y, t):
        if X >= 2 * self.two_q or Y >= 2 * self.two_q:
            self.events["range"] += 1
        if X == self.two_q:
            self.events["fold_eq"] += 1
        x = X - self.two_q if self._ge("fwd_fold", X, self.two_q) else X
        v = self.mulmod(Y, t)
        return (x + v) & M64, (x - v + self.two_q) & M64

    def _inv_head(self, X, Y):
        if X >= self.two_q or Y >= self.two_q:
            self.events["range"] += 1
        s = (X + Y) & M64
        if s == self.two_q:
            self.events["sum_eq"] += 1
        return s, (X - Y + self.two_q) & M64

    def bfly_inv(self, X, Y, t):
        s, d = self._inv_head(X, Y)
        return (s - self.two_q if self._ge("inv_sum", s, self.two_q) else s), self.mulmod(d, t)

    def bfly_inv_scaled(self, X, Y):
        s, d = self._inv_head(X, Y)
        return self.mulmod(s, self.n), self.mulmod(d, self.wn)

    def canonical(self, x):
        for k, name in ((1, "final_q"), (2, "final_2q"), (3, "final_3q")):
            if x == k * self.q:
                self.events[name] += 1
        x = x - self.two_q if self._ge("canon1", x, self.two_q) else x
        return x - self.q if self._ge("canon2", x, self.q) else x

    def barrett128(self, x):
        qhat = (x * self.ratio) >> 128
        r = (x - qhat * self.q) & M64
        if r == self.q:
            self.events["barrett_q"] += 1
        r = r - self.q if self._ge("barrett1", r, self.q) else r
        return r - self.q if self._ge("barrett2", r, self.q) else r

    def mulvar_lazy(self, a, b):
        return self.barrett128(a * b)

    def load(self, vec):
        """the ABI's entry: a word at or above q is reduced first"""
        return [int(x) % self.q for x in vec]

    def forward_lazy(self, a, stages=None):
        N, logn = self.L.N, self.L.logn
        for s in range(logn if stages is None else stages):
            m, t = 1 << s, N >> (s + 1)
            for i in range(m):
                tw, base = self.fwd[m + i], 2 * i * t
                for j in range(base, base + t):
                    a[j], a[j + t] = self.bfly_fwd(a[j], a[j + t], tw)
        return a

    def inverse_lazy(self, a):
        """to the words handed to canonical()"""
        N, logn = self.L.N, self.L.logn
        for s in range(logn - 1, 0, -1):
            m, t = 1 << s, N >> (s + 1)
            for i in range(m):
                tw, base = self.inv[m + i], 2 * i * t
                for j in range(base, base + t):
                    a[j], a[j + t] = self.bfly_inv(a[j], a[j + t], tw)
        for j in range(N // 2):
            a[j], a[j + N // 2] = self.bfly_inv_scaled(a[j], a[j + N // 2])
        return a

    def forward(self, vec):
        return [self.canonical(x) for x in self.forward_lazy(self.load(vec))]

    def inverse(self, vec):
        return [self.canonical(x) for x in self.inverse_lazy(self.load(vec))]

    def polymul(self, a, b):
        """the fused product: the two forward transforms multiplied as the lazy words they are, one barrett128 step each, and the
        inverse entered from its canonical results"""
        fa, fb = self.forward_lazy(self.load(a)), self.forward_lazy(self.load(b))
        return [self.canonical(x) for x in self.inverse_lazy([self.mulvar_lazy(x, y) for x, y in zip(fa, fb)])]
