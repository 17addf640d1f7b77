"""Adversarial inputs for the exact RNS base conversion, in Python integers only.

The conversion computes the mixed-radix digits c_l of x over the input base (x = c_0 + c_1 p_0 + c_2 p_0 p_1 + ...) and then
x mod q_o = sum_l c_l E_lo, E_lo = p_0 ... p_{l-1} mod q_o.  Any digit vector with 0 <= c_l < p_l belongs to exactly one residue
column, so a test can dictate the digits a kernel holds internally: residues_from_digits() builds the column.

The fixed-size FP64 kernels split digit and constant into halves of 25 bits, c = c1 2^25 + c0 and E = e1 2^25 + e0 with the low
half centred (round to nearest, ties to even: |c0|, |e0| <= 2^24), and accumulate three sums
    S2 += c1 e1,   S1 += c1 e0 + c0 e1,   S0 += c0 e0.
worst_columns() picks digits that drive each of these sums, and the split itself, to its largest magnitude.  split_constants() and
split() restate the halves as fhe_baseconv_create documents them; they serve to DESIGN inputs and to report the magnitudes reached,
never to form an expected value: that is exact_reference(), which knows nothing of halves.

Nothing here imports the kernels, the package or the oracle.
"""

HALF_BITS = 25
HALF = 1 << HALF_BITS
TIE = 1 << (HALF_BITS - 1)


def _prefix_products(mod_in):
    """Pi_{i<l} p_i for l = 0 .. m - 1"""
    out, prod = [], 1
    for p in mod_in:
        out.append(prod)
        prod *= p
    return out


def residues_from_digits(mod_in, digits):
    """r_j = (sum_l c_l Pi_{i<l} p_i) mod p_j"""
    assert len(digits) == len(mod_in) and all(0 <= c < p for c, p in zip(digits, mod_in))
    x = sum(c * w for c, w in zip(digits, _prefix_products(mod_in)))
    return [x % p for p in mod_in]


def exact_reference(mod_in, mod_out, residues):
    """-> (mixed-radix digits of the x in [0, P) with these residues, [x mod q_o])"""
    assert len(residues) == len(mod_in) and all(0 <= r < p for r, p in zip(residues, mod_in))
    digits, x, prod = [], 0, 1
    for r, p in zip(residues, mod_in):
        c = (r - x) * pow(prod, -1, p) % p          # x + c prod = r (mod p)
        digits.append(c)
        x += c * prod
        prod *= p
    return digits, [x % q for q in mod_out]


def split(v):
    """v = hi 2^25 + lo with hi = v / 2^25 rounded to nearest, ties to even (what rint does); |lo| <= 2^24"""
    hi = (v + TIE) >> HALF_BITS
    lo = v - hi * HALF
    if lo == -TIE and hi & 1:                    # the tie went up to an odd quotient: down to the even one
        hi, lo = hi - 1, TIE
    return hi, lo


def split_constants(mod_in, q):
    """-> [(E_l, e1_l, e0_l)], E_l = Pi_{i<l} p_i mod q"""
    out = []
    for w in _prefix_products(mod_in):
        E = w % q
        e1, e0 = split(E)
        out.append((E, e1, e0))
    return out


def split_sums(mod_in, q, digits, terms=None):
    """exact integers (S2, S1, S0) over the first `terms` limbs (all by default), nothing folded"""
    S2 = S1 = S0 = 0
    for (_, e1, e0), c in list(zip(split_constants(mod_in, q), digits))[:terms]:
        c1, c0 = split(c)
        S2 += c1 * e1
        S1 += c1 * e0 + c0 * e1
        S0 += c0 * e0
    return S2, S1, S0


def _clamp(c, p):
    return min(max(c, 0), p - 1)


def _candidates(p):
    """digits whose high half is extreme (largest, or 0 .. 2) and whose low half is at or next to +-2^24, clamped into [0, p)"""
    top = split(p - 1)[0]
    out = {0, p - 1}
    for c1 in (top, top - 1, top - 2, 0, 1, 2):
        for c0 in (TIE, TIE - 1, -TIE, -TIE + 1, 0):
            out.add(_clamp(c1 * HALF + c0, p))
    return sorted(out)


def _best(p, score):
    """the candidate digit with the largest score(c1, c0); ties go to the larger digit"""
    return max(_candidates(p), key=lambda c: (score(*split(c)), c))


def worst_columns(mod_in, mod_out):
    """-> [(name, digits)]: digit vectors, each named for what it drives to its edge"""
    m = len(mod_in)
    cols = [("zero", [0] * m), ("max", [p - 1 for p in mod_in])]
    for o, q in enumerate(mod_out):
        ks = split_constants(mod_in, q)
        for sign, tag in ((1, "+"), (-1, "-")):
            # every term c1 e0 + c0 e1 as far to this side as a digit of [0, p) can push it: c0 = sign 2^24 (e1 >= 0), and the largest
            # c1 where e0 is on this side, the smallest where it is not
            cols.append((f"S1{tag}[{o}]", [_best(p, lambda c1, c0, e1=e1, e0=e0: sign * (c1 * e0 + c0 * e1)) for p, (_, e1, e0) in zip(mod_in, ks)]))
        # c0 = sign(e0) 2^24: every term of S0 at +2^48 scale; among those the largest c1
        cols.append((f"S0[{o}]", [_best(p, lambda c1, c0, e0=e0: (c0 * e0, c1)) for p, (_, _, e0) in zip(mod_in, ks)]))
    # the tie of the split: c = t 2^25 + 2^24 goes to the even neighbour, c0 = +2^24 for even t and -2^24 for odd t
    for tag, parity in (("even", 0), ("odd", 1)):
        digs = []
        for p in mod_in:
            t = (p - 1 - TIE) >> HALF_BITS
            t -= (t & 1) != parity
            digs.append(_clamp(t * HALF + TIE, p))
        cols.append((f"tie-{tag}", digs))
    for l in range(m):
        cols.append((f"single[{l}]", [mod_in[l] - 1 if j == l else 0 for j in range(m)]))
    for phase in (0, 1):
        cols.append((f"alternate{phase}", [p - 1 if (j + phase) & 1 else 0 for j, p in enumerate(mod_in)]))
    for name, digs in cols:
        assert all(0 <= c < p for c, p in zip(digs, mod_in)), name
    return cols


def worst_residues(mod_in, mod_out):
    """-> (names, residue columns [n_w][m], expected words [n_w][k]) of worst_columns(), the expected words from exact_reference()"""
    names, res, want = [], [], []
    for name, digs in worst_columns(mod_in, mod_out):
        r = residues_from_digits(mod_in, digs)
        got_digs, words = exact_reference(mod_in, mod_out, r)
        assert got_digs == digs, name
        names.append(name)
        res.append(r)
        want.append(words)
    return names, res, want
