"""The round-to-nearest rescale in Python, written twice, and what the tests of it share.

Definition (include/fhe_mi355x.h, fhe_rescale).  For one part let C in [0, Q) be the CRT lift over q_0 .. q_{L-1} of one
coefficient of the part's coefficient form, q = q_{L-1} (odd), h = (q - 1) / 2.
    floor:    (C - [C]_q) / q,  [C]_q in [0, q)
    nearest:  floor((C + h) / q) = (C - r) / q,  r = [C]_q if [C]_q <= h else [C]_q - q,  r in [-h, h]  (no ties: q is odd)
Output limb j < L-1 is the canonical word of NTT_j((c_j - (r mod q_j)) q^-1 mod q_j).

round_rescale_ref is (a): per limb, the centred remainder on the oracle's transforms.  round_rescale_int is (b): Python integers,
CRT lift, (C + h) // q, residues, forward transform.  They share the oracle's transforms and nothing else; tests/
test_rescale_round_ref.py holds (a) against (b) and, with nearest = False, against oracle.keyswitch_ref.rescale_ref.

The SEAL sequence (RNSTool::divide_and_round_q_last_ntt_inplace: add h to the last limb modulo q, reduce modulo q_j, subtract h mod
q_j, subtract from c_j, multiply by q^-1) yields the same residues, since (y + h mod q) - h = r; SEAL itself is not at hand, so
the words are pinned by the integer definition only.

Decryption bound (derived, not fitted).  The input parts decrypt to v = sum_i c_i s^i (centred, over Q).  Per part the rescale
removes r_i with |r_i| <= h coefficient by coefficient, so over Q / q
    q dec' = v - sum_i r_i s^i,    |(r_i s^i)[k]| <= h |s^i|_1,
and with div_round(v, q) = (v - rho) / q, |rho| <= h:
    |dec' - div_round(v, q)| = |rho - sum_i r_i s^i| / q <= (h / q) (1 + sum_i |s^i|_1) < 1/2 (1 + sum_i |s^i|_1).
For a two-part ciphertext that is 1/2 (1 + 1 + |s|_1): the issue's "1/2 (1 + |s|_1)" per removed remainder, plus the rounding of
the comparison value itself.  The flooring rescale has |delta_i| < q instead of <= h: twice the bound, and a bias of mean q / 2.
"""
import numpy as np

from oracle import cport as O
from oracle import keyswitch_ref as KR

from . import rlwe

U = np.uint64


def round_rescale_ref(parts, qs, L, logn, nearest=True):
    """(a): parts (n, L, N) NTT domain -> (n, L-1, N); per limb, the centred remainder of the last limb"""
    qs = [int(q) for q in qs[:L]]
    ql, N = qs[L - 1], 1 << logn
    h = (ql - 1) // 2
    rps = KR._tables(qs, logn)
    out = []
    for c in parts:
        c = np.asarray(c, dtype=U)
        y = O.nwt_inverse(c[L - 1], ql, rps[L - 1])
        neg = (y > U(h)) if nearest else np.zeros(N, dtype=bool)
        mag = np.where(neg, U(ql) - y, y)                                     # |r|
        delta = np.stack([np.where(neg, (U(q) - mag % U(q)) % U(q), mag % U(q)) for q in qs[:L - 1]])
        dn = O.nwt_forward_batch(delta, qs[:L - 1], rps[:L - 1])
        r = np.zeros((L - 1, N), dtype=U)
        for j in range(L - 1):
            qj = U(qs[j])
            r[j] = O.modmul((c[j] % qj + (qj - dn[j])) % qj, np.full(N, pow(ql % qs[j], -1, qs[j]), dtype=U), qs[j])
        out.append(r)
    return np.stack(out)


def lift(part, qs, logn):
    """one part (L, N), NTT domain -> its coefficients as Python ints in [0, Q)"""
    qs = [int(q) for q in qs]
    Q = rlwe.prod(qs)
    coef = O.nwt_inverse_batch(np.asarray(part, dtype=U), qs, KR._tables(qs, logn))
    acc = [0] * coef.shape[1]
    for j, q in enumerate(qs):
        Mj = Q // q
        w = Mj * pow(Mj, -1, q) % Q
        acc = [(a + int(x) * w) % Q for a, x in zip(acc, coef[j])]
    return acc


def rescaled_ints(C, q, nearest):
    """the rescaled coefficients as integers"""
    h = (q - 1) // 2
    return [(c + h) // q if nearest else c // q for c in C]


def round_rescale_int(parts, qs, L, logn, nearest=True):
    """(b): Python integers -- CRT lift, (C + h) // q, residues, forward transform"""
    qs = [int(q) for q in qs[:L]]
    out = []
    for c in parts:
        ints = rescaled_ints(lift(c, qs, logn), qs[L - 1], nearest)
        out.append(rlwe.to_ntt(ints, qs[:L - 1]))
    return np.stack(out)


def l1_powers(s, n_parts):
    """|s^i|_1 for i < n_parts (s^0 = 1)"""
    out, p = [1], None
    for _ in range(1, n_parts):
        p = list(s) if p is None else rlwe.negacyclic_mul_int(p, s)
        out.append(sum(abs(int(x)) for x in p))
    return out


def nearest_bound_2x(s, n_parts):
    """TWICE the bound on |dec' - div_round(v, q)| of the nearest rescale (module docstring), an integer: 1 + sum_i |s^i|_1"""
    return 1 + sum(l1_powers(s, n_parts))


# ------------------------------------------------------------------------------------------------ inputs that dictate the branch
def branch_words(q):
    """the last-limb coefficients at which the centring switches, and its ends"""
    h = (q - 1) // 2
    return [0, 1, h - 1, h, h + 1, q - 1]


def branch_positions(N, tile_cols=16):
    """where they go: the ends of the limb, and the two sides of the first column-tile boundary (16 columns at the two-launch sizes)"""
    pos = [0, 1, N - 1]
    if N > 2 * tile_cols:
        pos += [tile_cols - 1, tile_cols]
    return pos


def last_limb(y, q, logn):
    """the NTT-domain limb whose coefficient form is y"""
    return O.nwt_forward(np.asarray(y, dtype=U), int(q), O.root_powers(int(q), logn))


def dictated_parts(qs, L, logn, n_parts, seed, fill=None):
    """(n_parts, L, N) NTT-domain parts: random limbs below L-1; the last limb is the transform of a y that carries every branch word
    at every branch position in turn (part p starts the cycle at word p) and random words between -- or, with fill, y = fill everywhere"""
    qs = [int(q) for q in qs[:L]]
    N, q = 1 << logn, qs[L - 1]
    rng = np.random.default_rng(seed)
    parts = np.zeros((n_parts, L, N), dtype=U)
    words, pos = branch_words(q), branch_positions(N)
    for p in range(n_parts):
        for j in range(L - 1):
            parts[p, j] = rng.integers(0, qs[j], N, dtype=U)
        if fill is not None:
            y = np.full(N, fill, dtype=U)
        else:
            y = rng.integers(0, q, N, dtype=U)
            for k, at in enumerate(pos):
                y[at] = words[(p + k) % len(words)]
            # every word once more, next to each other, past the second tile
            base = min(N - len(words), 40)
            if base > pos[-1] or N <= 32:
                for k, w in enumerate(words):
                    if base + k not in pos:
                        y[base + k] = w
        parts[p, L - 1] = last_limb(y, q, logn)
    return parts
