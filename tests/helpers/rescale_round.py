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


# Row length 2^PR of the column pass's 2^PC x 2^PR matrix at the two-launch sizes, and the width of a column tile: data copied from
# fhe_reliability_gpu_amd/csrc/ntt_plan.hpp (Plan<LOGN>::Row::P = 8, 8, 8, 8, 9 for LOGN 13..17; PlanGeom<LOGN, 1>::TC = 16).  Nothing
# asserts the plan: the table only says which input word reaches which tile of which row.
ROW_LEN = {13: 256, 14: 256, 15: 256, 16: 256, 17: 512}
TILE_COLS = 16


def branch_positions(N, tile_cols=16, row_len=None):
    """where they go: the ends of the limb, and the two sides of the first column-tile boundary (16 columns at the two-launch sizes).
    With row_len, after those: the first word of row 1 and the two sides of its first tile boundary, then the first word of the last
    row and the two sides of its last tile boundary (its last word, N - 1, is there already)"""
    pos = [0, 1, N - 1]
    if N > 2 * tile_cols:
        pos += [tile_cols - 1, tile_cols]
    if row_len is not None:
        pos += [row_len, row_len + tile_cols - 1, row_len + tile_cols, N - row_len, N - tile_cols - 1, N - tile_cols]
    return pos


def position_classes(N, row_len, tile_cols=16):
    """the positions of branch_positions(N, tile_cols, row_len) by what they probe: a class is the unit over which the parts of a
    three-part case carry every branch word (first_word)"""
    return {"row start": [0, row_len, N - row_len],
            "left of a tile boundary": [tile_cols - 1, row_len + tile_cols - 1, N - tile_cols - 1],
            "right of a tile boundary": [tile_cols, row_len + tile_cols, N - tile_cols],
            "row 0": [0, 1, tile_cols - 1, tile_cols],
            "row 1": [row_len, row_len + tile_cols - 1, row_len + tile_cols],
            "last row": [N - row_len, N - tile_cols - 1, N - tile_cols, N - 1]}


def first_word(k, n_base):
    """index of the branch word that part 0 puts at position number k (part p: p further on, cyclically).  The n_base positions
    without row_len count up, as they always did: 0, 1, N-1, 15, 16 start at words 0, 1, 2, 3, 4.  A position that row_len adds starts
    three words away from its counterpart in row 0 -- row starts at 3 (0 has 0), left sides at 0 (15 has 3), right sides at 1 (16 has
    4) -- so that over three parts, which give a position three consecutive words, the pair sees all six"""
    return k if k < n_base else (3, 0, 1)[(k - n_base) % 3]


def last_limb(y, q, logn):
    """the NTT-domain limb whose coefficient form is y"""
    return O.nwt_forward(np.asarray(y, dtype=U), int(q), O.root_powers(int(q), logn))


def dictated_y(q, logn, p, rng, row_len=None):
    """the coefficient form of part p's last limb: the branch words at the branch positions, random words between"""
    N = 1 << logn
    words, pos, n_base = branch_words(q), branch_positions(N, row_len=row_len), len(branch_positions(N))
    y = rng.integers(0, q, N, dtype=U)
    for k, at in enumerate(pos):
        y[at] = words[(p + first_word(k, n_base)) % len(words)]
    # every word once more, next to each other, past the second tile
    base = min(N - len(words), 40)
    if base > pos[n_base - 1] or N <= 32:
        for k, w in enumerate(words):
            if base + k not in pos:
                y[base + k] = w
    return y


def dictated_parts(qs, L, logn, n_parts, seed, fill=None, row_len=None):
    """(n_parts, L, N) NTT-domain parts: random limbs below L-1; the last limb is the transform of a y that carries every branch word
    at every branch position in turn (part p starts the cycle at word p) and random words between -- or, with fill, y = fill everywhere.
    row_len adds the positions in row 1 and in the last row of the column pass's matrix (branch_positions); without it the parts are
    what they were before the argument existed"""
    qs = [int(q) for q in qs[:L]]
    N, q = 1 << logn, qs[L - 1]
    rng = np.random.default_rng(seed)
    parts = np.zeros((n_parts, L, N), dtype=U)
    for p in range(n_parts):
        for j in range(L - 1):
            parts[p, j] = rng.integers(0, qs[j], N, dtype=U)
        y = np.full(N, fill, dtype=U) if fill is not None else dictated_y(q, logn, p, rng, row_len)
        parts[p, L - 1] = last_limb(y, q, logn)
    return parts


# ------------------------------------------------------------------------------------------------ limb layouts, and what every case is held to
# ciphertext primes, then the size of the special primes.  L = 3: the two remaining limbs are one run of one arithmetic path
PRIME_SETS = {"50": ([50, 50, 50], 50), "61": ([61, 61, 61], 61), "50+61last": ([50, 50, 61], 50), "61+50last": ([61, 61, 50], 61),
              "30+61last": ([30, 30, 61], 61)}
# L = 5, the paths alternating: the four remaining limbs are four runs of one limb each (for_each_run: off = 0 .. 3)
ALTERNATING = {"50/61/50/61/50": ([50, 61, 50, 61, 50], 61), "61/50/61/50/61": ([61, 50, 61, 50, 61], 50)}


def limb_bits(kind, K):
    """the bit sizes of a named layout's ciphertext primes followed by its K special primes"""
    bits, sp = (PRIME_SETS.get(kind) or ALTERNATING[kind])
    return bits + [sp] * K


def moduli(F, logn, kind, K):
    return F.create_moduli(1 << logn, limb_bits(kind, K))


def random_parts(qs, L, logn, n_parts, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.stack([rng.integers(0, int(q), 1 << logn, dtype=U) for q in qs[:L]]) for _ in range(n_parts)])


def references(parts, qs, L, logn, differs=True, what=""):
    """(nearest, floor) of one case: statement (a), the oracle's rescale, and the condition that makes the nearest words tell"""
    near, floor = round_rescale_ref(parts, qs, L, logn, True), KR.rescale_ref(parts, qs, L, logn)
    if differs:
        assert_every_tile_differs(near, floor, what)
    else:
        assert (near == floor).all(), what
    return near, floor


def assert_every_tile_differs(near, floor, what="", tile_cols=TILE_COLS):
    """in every 16-column tile of every output limb of every part the nearest words differ from the flooring words somewhere: a tile
    computed by the flooring form cannot pass a comparison with ``near``"""
    tiles = (near != floor).reshape(near.shape[:-1] + (-1, tile_cols)).any(axis=-1)
    assert tiles.all(), f"{what}: nearest equals floor on {int((~tiles).sum())} of {tiles.size} tiles, first (part, limb, tile) {np.argwhere(~tiles)[0].tolist()}"


def same(got, want, what):
    got = got.download().reshape(want.shape)
    assert (got == want).all(), f"{what}: {int((got != want).sum())} words differ, first at {np.argwhere(got != want)[0].tolist()}"


# ------------------------------------------------------------------------------------------------ fhe_hmult
def hmult_case(F, logn, kind, L, K, dnum, seed):
    qs = moduli(F, logn, kind, K)
    N = 1 << logn
    rng = np.random.default_rng(seed)
    rnd = lambda qq: np.stack([rng.integers(0, q, N, dtype=U) for q in qq])
    a0, a1, b0, b1 = (rnd(qs[:L]) for _ in range(4))
    key = np.stack([np.stack([rnd(qs) for _ in range(2)]) for _ in range(dnum)])
    return qs, a0, a1, b0, b1, key


def hmult_relin_ref(qs, a0, a1, b0, b1, key, L, K, dnum, logn):
    """the relinearised product before its rescale, (2, L, N)"""
    d0, d1, d2 = KR.tensor_ref(a0, a1, b0, b1, qs)
    return np.stack(KR.keyswitch_ref(d2, key, qs, L, K, dnum, logn, add0=d0, add1=d1))


def hmult_want(qs, a0, a1, b0, b1, key, L, K, dnum, logn, nearest):
    r = round_rescale_ref(hmult_relin_ref(qs, a0, a1, b0, b1, key, L, K, dnum, logn), qs, L, logn, nearest)
    return r[0], r[1]
