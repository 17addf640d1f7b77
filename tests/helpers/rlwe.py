"""A small RLWE toolkit in Python integers: keys, encryption, decryption and worst-case noise bounds for the tests that hold the
composites at the DECRYPTION level (decrypt the result, compare plaintexts) instead of word for word.

oracle/keyswitch_ref.py restates the engine's sequence of steps; a mistake in the sequence itself is made on both sides.  What
is here shares nothing with that sequence: it knows the ring Z[X] / (X^N + 1), the secret, and what a ciphertext has to decrypt
to.  The oracle's transforms (oracle.cport) serve for per-limb negacyclic products only; nothing of the engine is imported and no
constant of any plan is kept: every function takes its moduli.

Conventions.  Polynomials that carry meaning (secrets, messages, errors, decrypted values) are lists of Python ints, coefficient
order.  Ciphertext parts and keys are numpy uint64 arrays of residues in the NTT domain, [limbs][N], the layout the engine and
the oracle composites take.  t = 0 is the CKKS form (error E = e), t > 0 the BGV form (E = t e, plaintexts modulo t); |e| <= ERR.

Noise bounds (worst case, not probabilistic; |s|_inf <= 1, so |a s|_inf <= N |a|_inf for every a, and |a s^2|_inf <= N^2 |a|_inf).
E_unit is 1 (CKKS) or t (BGV).

* fresh: decrypt(encrypt(m)) = m + E, |E| <= E_unit ERR.

* key switch.  With evk_d = (-a_d s + E_d + P Qhat_d [Qhat_d^-1]_{Q_d} s_from, a_d) and ext_d the integer lift of the digit
  [c]_{Q_d} (0 <= ext_d < Q_d, whatever automorphism is applied to it), the sums are
      acc_0 + acc_1 s = P c s_from + E_unit sum_d ext_d e_d   (mod P Q),
  because sum_d ext_d Qhat_d [Qhat_d^-1]_{Q_d} = c (mod Q).  The mod-down takes delta_h = acc_h (mod P) away and divides by P
  exactly, with |delta_h| < P (CKKS: delta = [acc]_P) or |delta_h| < t P (BGV: delta = t [acc t^-1]_P, a multiple of t), so
      out_0 + out_1 s = c s_from + E',   E' = (E_unit sum_d ext_d e_d - delta_0 - delta_1 s) / P   (mod Q)
  and |E'| <= E_unit (dnum N ERR max_d Q_d / P + N + 1) + 1.  In the BGV form P E' is a multiple of t and P is a unit modulo t:
  E' = 0 (mod t), coefficient by coefficient.

* rotation: (sigma(c0) + ks_0, ks_1) with the key switch of sigma(c1) from sigma(s): decrypts to sigma(v) + E' where v is what
  the input decrypts to; sigma permutes coefficients and flips signs, so the error is bounded by |error of v| + key-switch bound,
  and is 0 modulo t in the BGV form.  A hoisted rotation applies sigma to the extended digits instead; 0 <= |sigma(ext_d)| < Q_d
  still holds and the bound is the same.

* rescale / mod switch of n parts: c'_i = (c_i - delta_i) / q_last with delta_i = c_i (mod q_last), |delta_i| < E_unit q_last
  (CKKS: [c_i]_{q_last}; BGV: t [c_i t^-1]_{q_last}).  If the input decrypts to v (centred, over Q) then over Q / q_last
      q_last dec' = v - sum_i delta_i s^i,   |dec' - v / q_last| <= E_unit sum_{i<n} N^i < that + 1 = noise_bound_rescale.
  BGV: q_last dec' = v (mod t), so dec' = q_last^-1 m (mod t) exactly.

* tensor: d0 + d1 s + d2 s^2 = (a0 + a1 s)(b0 + b1 s) (mod Q): three parts decrypt to v1 v2 with NO added error as long as
  N |v1| |v2| < Q / 2.  Against m1 m2 the error is m1 E2 + m2 E1 + E1 E2, at most N (|m1| B2 + |m2| B1 + B1 B2).

* multiply: tensor, relinearisation (key switch of d2 from s^2, plus d0 / d1: v1 v2 + E'), optional rescale: the sums of the above.

* BSGS product y = sum_g sigma_G(sum_b diag[g][b] R_b), R_0 = x, R_b a (hoisted) rotation of x: R_b carries the input's error and,
  for b > 0, one key-switch error; a product with a diagonal of entries below D multiplies an error by at most N D; each giant
  rotation (g > 0) adds one key-switch error: n2 N D (n1 B_in + (n1 - 1) B_ks) + (n2 - 1) B_ks.

These are derived bounds; they are not tuned to what any implementation returns.
"""
import functools
import random

import numpy as np

from oracle import cport as O

U = np.uint64
ERR = 4          # |e| <= ERR for every fresh error polynomial


# ------------------------------------------------------------------------------------------------ integers
def prod(xs):
    out = 1
    for x in xs:
        out *= int(x)
    return out


def centred(x, mod):
    """the representative of x modulo mod in (-mod / 2, mod / 2]"""
    x %= mod
    return x - mod if x > mod // 2 else x


def sigma_int(poly, k):
    """X -> X^k on an integer polynomial modulo X^N + 1 (k odd)"""
    N = len(poly)
    out = [0] * N
    for i, v in enumerate(poly):
        j = (i * k) % (2 * N)
        if j >= N:
            out[j - N] = -v
        else:
            out[j] = v
    return out


@functools.lru_cache(maxsize=None)
def _table(q, logn):
    return O.root_powers(q, logn)


def _tables(qs, logn):
    return np.stack([_table(int(q), logn) for q in qs])


def _col(qs):
    return np.array([int(q) for q in qs], dtype=U)[:, None]


def residues(poly, qs):
    """integer polynomial -> [len(qs)][N] canonical residues (coefficient domain)"""
    p = np.array([int(x) for x in poly], dtype=object)
    return np.stack([(p % int(q)).astype(U) for q in qs])


def ntt(x, qs):
    x = np.asarray(x, dtype=U)
    return O.nwt_forward_batch(x, [int(q) for q in qs], _tables(qs, x.shape[1].bit_length() - 1))


def intt(x, qs):
    x = np.asarray(x, dtype=U)
    return O.nwt_inverse_batch(x, [int(q) for q in qs], _tables(qs, x.shape[1].bit_length() - 1))


def to_ntt(poly, qs):
    """integer polynomial -> NTT-domain residues [len(qs)][N]"""
    return ntt(residues(poly, qs), qs)


def _mul(a, b, qs):
    return O.modmul_batch(a, b, [int(q) for q in qs])


def _add(a, b, qs):
    return (np.asarray(a, dtype=U) + np.asarray(b, dtype=U)) % _col(qs)


def _sub(a, b, qs):
    q = _col(qs)
    return (np.asarray(a, dtype=U) + (q - np.asarray(b, dtype=U) % q)) % q


def _scale(a, c, qs):
    """a times the integer c, limb by limb"""
    N = a.shape[1]
    return np.stack([O.modmul(a[j], np.full(N, int(c) % int(q), dtype=U), int(q)) for j, q in enumerate(qs)])


def crt_centred(res, qs):
    """[limbs][N] residues (coefficient domain) -> centred Python ints modulo prod(qs)"""
    Q = prod(qs)
    acc = np.zeros(res.shape[1], dtype=object)
    for j, q in enumerate(qs):
        Mj = Q // int(q)
        acc = acc + res[j].astype(object) * (Mj * pow(Mj, -1, int(q)) % Q)
    return [centred(int(x), Q) for x in acc]


@functools.lru_cache(maxsize=None)
def _work_primes(N, count):
    return tuple(O.gen_primes(N, 59, count))


def negacyclic_mul_int(a, b, mod=0):
    """a b modulo X^N + 1 over Z (exact: residues at enough 59-bit primes to hold N |a| |b|, then CRT); with mod, reduced into [0, mod)"""
    N = len(a)
    bound = N * max(abs(int(x)) for x in a) * max(abs(int(x)) for x in b)
    if bound == 0:
        return [0] * N
    count = 1
    while prod(_work_primes(N, count)) <= 2 * bound:
        count += 1
    ps = list(_work_primes(N, count))
    out = crt_centred(intt(_mul(to_ntt(a, ps), to_ntt(b, ps), ps), ps), ps)
    return [x % mod for x in out] if mod else out


# ------------------------------------------------------------------------------------------------ the scheme
def keygen(N, rnd):
    """a ternary secret from a seeded random.Random"""
    return [rnd.choice((-1, 0, 1)) for _ in range(N)]


def _uniform(qs, N, rnd):
    g = np.random.default_rng(rnd.getrandbits(64))
    return np.stack([g.integers(0, int(q), N, dtype=U) for q in qs])


def _error(N, rnd, t):
    return [(t if t else 1) * rnd.randint(-ERR, ERR) for _ in range(N)]


def switching_key(s_from, s, qs, L, K, dnum, t=0, rnd=None):
    """[dnum][2][L+K][N], NTT domain: (-a_d s + E_d + P Qhat_d [Qhat_d^-1]_{Q_d} s_from, a_d), E_d = e_d (t = 0) or t e_d, |e_d| <= ERR.
    s_from = s^2 gives a relinearisation key, s_from = sigma_k(s) the Galois key of k."""
    rnd = rnd or random.Random(0)
    qs = [int(q) for q in qs[:L + K]]
    N, Q, P = len(s), prod(qs[:L]), prod(qs[L:])
    alpha = -(-L // dnum)
    s_n, from_n = to_ntt(s, qs), to_ntt(s_from, qs)
    key = np.zeros((dnum, 2, L + K, N), dtype=U)
    for d in range(dnum):
        Qd = prod(qs[d * alpha:min(L, (d + 1) * alpha)])
        Qhat = Q // Qd
        factor = P * Qhat * pow(Qhat, -1, Qd)
        a = _uniform(qs, N, rnd)
        key[d, 0] = _add(_sub(to_ntt(_error(N, rnd, t), qs), _mul(a, s_n, qs), qs), _scale(from_n, factor, qs), qs)
        key[d, 1] = a
    return key


def encrypt(m, s, qs, t=0, rnd=None):
    """symmetric: c1 uniform, c0 = m + E - c1 s; (c0, c1), NTT domain, over the primes qs"""
    rnd = rnd or random.Random(0)
    qs = [int(q) for q in qs]
    N = len(s)
    c1 = _uniform(qs, N, rnd)
    E = _error(N, rnd, t)
    c0 = _sub(to_ntt([int(x) + e for x, e in zip(m, E)], qs), _mul(c1, to_ntt(s, qs), qs), qs)
    return c0, c1


def decrypt(parts, s, qs):
    """sum_i parts[i] s^i per limb, CRT to a centred integer polynomial over prod(qs); parts in the NTT domain, any number of them"""
    qs = [int(q) for q in qs]
    s_n = to_ntt(s, qs)
    acc, power = np.asarray(parts[0], dtype=U) % _col(qs), None
    for c in parts[1:]:
        power = s_n if power is None else _mul(power, s_n, qs)
        acc = _add(acc, _mul(np.asarray(c, dtype=U), power, qs), qs)
    return crt_centred(intt(acc, qs), qs)


def keyswitch_error(out0, out1, c, s, s_from, qs):
    """out0 + out1 s - c s_from as a centred integer polynomial over prod(qs): what a key switch of c from s_from to s added"""
    qs = [int(q) for q in qs]
    r = _add(out0, _mul(out1, to_ntt(s, qs), qs), qs)
    r = _sub(r, _mul(c, to_ntt(s_from, qs), qs), qs)
    return crt_centred(intt(r, qs), qs)


class Party:
    """One secret over the moduli of a plan (qs = L ciphertext primes then K special ones, handed in by the caller), its keys on demand,
    and the bounds of that plan; t = 0 for the CKKS form.  Everything random comes from one seeded random.Random."""

    def __init__(self, N, qs, L, K, dnum, t=0, seed=0):
        self.N, self.logn = N, N.bit_length() - 1
        self.qs, self.L, self.K, self.dnum, self.t = [int(q) for q in qs[:L + K]], L, K, dnum, t
        self.rnd = random.Random(seed)
        self._keys = {}
        self.s = keygen(N, self.rnd)
        self.s2 = negacyclic_mul_int(self.s, self.s)
        self.Q = prod(self.qs[:L])
        self.b_fresh = noise_bound_fresh(t)
        self.b_ks = noise_bound_keyswitch(N, self.qs, L, K, dnum, t)

    def relin_key(self):
        if "relin" not in self._keys:
            self._keys["relin"] = switching_key(self.s2, self.s, self.qs, self.L, self.K, self.dnum, self.t, self.rnd)
        return self._keys["relin"]

    def galois_key(self, k):
        if k not in self._keys:
            self._keys[k] = switching_key(sigma_int(self.s, k), self.s, self.qs, self.L, self.K, self.dnum, self.t, self.rnd)
        return self._keys[k]

    def message(self, below=None):
        """uniform in [0, below) (default: [0, t))"""
        return [self.rnd.randrange(below or self.t) for _ in range(self.N)]

    def uniform(self, limbs=None):
        return _uniform(self.qs[:limbs or self.L], self.N, self.rnd)

    def encrypt(self, m):
        return encrypt(m, self.s, self.qs[:self.L], self.t, self.rnd)

    def decrypt(self, parts, limbs=None):
        return decrypt(parts, self.s, self.qs[:limbs or self.L])


# ------------------------------------------------------------------------------------------------ bounds (module docstring)
def _unit(t):
    return t if t else 1


def noise_bound_fresh(t=0):
    return _unit(t) * ERR


def noise_bound_keyswitch(N, qs, L, K, dnum, t=0):
    qs = [int(q) for q in qs[:L + K]]
    alpha = -(-L // dnum)
    Qd = max(prod(qs[d * alpha:min(L, (d + 1) * alpha)]) for d in range(dnum))
    P = prod(qs[L:])
    return _unit(t) * (-(-dnum * N * ERR * Qd // P) + N + 1) + 1


def noise_bound_rotate(b_in, b_ks):
    return b_in + b_ks


def noise_bound_rescale(N, n_parts, t=0):
    """on |dec' - v / q_last|: check it as |q_last dec' - v| <= q_last * bound, in integers"""
    return _unit(t) * sum(N ** i for i in range(n_parts)) + 1


def noise_bound_tensor(N, m1, m2, b1, b2):
    """on |decrypt(d0, d1, d2) - m1 m2| for inputs m_i + E_i, |m_i| <= m1 / m2, |E_i| <= b1 / b2"""
    return N * (m1 * b2 + m2 * b1 + b1 * b2)


def noise_bound_hmult(N, m1, m2, b1, b2, b_ks, q_last=0, t=0):
    """on |dec - m1 m2| without rescale; with q_last, on |q_last dec' - m1 m2| (divide by q_last for the error of dec' itself)"""
    b = noise_bound_tensor(N, m1, m2, b1, b2) + b_ks
    return b + q_last * noise_bound_rescale(N, 2, t) if q_last else b


def noise_bound_bsgs(N, n1, n2, diag_max, b_in, b_ks):
    return n2 * N * diag_max * (n1 * b_in + (n1 - 1) * b_ks) + (n2 - 1) * b_ks


# ------------------------------------------------------------------------------------------------ the properties
def assert_error(err, bound, t=0, what="error"):
    """every coefficient of err is within the bound and, in the BGV form, 0 modulo t; returns the number of coefficients checked"""
    if t:
        bad = [i for i, x in enumerate(err) if x % t]
        assert not bad, f"{what}: not 0 modulo t = {t} at {len(bad)} of {len(err)} coefficients (first at {bad[0]})"
    worst = max(abs(x) for x in err)
    assert worst <= bound, f"{what}: |error| reaches 2^{worst.bit_length()}, above the bound {bound} (2^{int(bound).bit_length()})"
    return len(err)


def assert_plaintext(dec, want, t, what="plaintext"):
    """dec = want modulo t at every coefficient, no tolerance; returns the number of coefficients checked"""
    assert len(dec) == len(want)
    bad = [i for i, (d, w) in enumerate(zip(dec, want)) if (d - w) % t]
    assert not bad, f"{what}: differs from the expected plaintext modulo t = {t} at {len(bad)} of {len(dec)} coefficients (first at {bad[0]})"
    return len(dec)


def assert_close(dec, want, bound, what="value"):
    """|dec - want| <= bound at every coefficient (the CKKS form); returns the number of coefficients checked"""
    assert len(dec) == len(want)
    worst = max(abs(d - w) for d, w in zip(dec, want))
    assert worst <= bound, f"{what}: off by 2^{worst.bit_length()}, above the bound {bound} (2^{int(bound).bit_length()})"
    return len(dec)


def assert_rescaled(dec_out, v_in, q_last, bound_in, n_parts, N, t=0, what="rescale"):
    """q_last dec' = v - sum_i delta_i s^i: the scaled error q_last dec' - v is within bound_in + q_last noise_bound_rescale (bound_in: how
    far v_in may be from what the input really decrypts to; 0 when v_in is that value itself) and, in the BGV form, 0 modulo t"""
    err = [q_last * d - v for d, v in zip(dec_out, v_in)]
    return assert_error(err, bound_in + q_last * noise_bound_rescale(N, n_parts, t), t, what)


def div_round(x, q):
    """round(x / q), halves away from zero, in integers"""
    return (2 * abs(x) + q) // (2 * q) * (1 if x >= 0 else -1)
