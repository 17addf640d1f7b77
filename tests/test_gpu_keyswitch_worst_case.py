"""Key switch, rotations, tensor, rescale and homomorphic multiply on inputs that dictate their internals
(tests/helpers/ks_worst_case.py): key words that put every product next to the rounding boundary of the FP64 quotient estimate
and every fold block of the lazy accumulator on one sign, 128-bit sums of (q - 1)^2, coefficients at the edges between
neighbouring primes, worst-case mixed-radix digits inside the key switch's own conversions, and an accumulator solved so that the
mod-down's tail and the rescale meet acc == conv, the borrow by one and v + add == q.  Every comparison is == against
oracle/keyswitch_ref.py; every checked call returns the same words and an all-zero flag buffer."""
import numpy as np
import pytest

from helpers import ks_worst_case as KW
from helpers.checked_plan import limb_bits

pytestmark = pytest.mark.gpu
U = np.uint64


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


def _bits(kind, L, K):
    return limb_bits({50: "50/50", 61: "61/61"}.get(kind, kind), L, K)


def _plan(F, eng, logn, L, K, dnum, kind):
    from oracle import cport as O
    qs = F.create_moduli(1 << logn, _bits(kind, L, K))
    t = eng.tables(logn, qs)
    rps = np.stack([O.root_powers(q, logn) for q in qs])
    return qs, rps, t, F.KeySwitch(eng, t, L, K, dnum), F.Abft(eng, t)


def _no_flag(flags, what=""):
    """every word of a (possibly nested) flag dictionary is there and zero"""
    assert flags is not None, f"{what}: no flags returned"
    if isinstance(flags, dict):
        assert flags, what
        for name, f in flags.items():
            _no_flag(f, f"{what}/{name}")
    elif isinstance(flags, (list, tuple)):
        assert len(flags), what
        for i, f in enumerate(flags):
            _no_flag(f, f"{what}[{i}]")
    else:
        f = np.asarray(flags)
        assert f.size, what
        assert not f.any(), f"{what}: flags {np.argwhere(f != 0).tolist()[:8]} = {f[f != 0].tolist()[:8]} on a clean run"


def _eq(got, want, what=""):
    assert len(got) == len(want), f"{what}: {len(got)} outputs for {len(want)}"
    for g, w in zip(got, want):
        g = g.download().reshape(w.shape)
        assert (g == w).all(), f"{what}: {int((g != w).sum())} words differ, first at {np.argwhere(g != w)[0].tolist()}"


def _sigma(x, k, qs, rps):
    """sigma_k of NTT-domain rows, through the coefficient domain as oracle/keyswitch_ref.py applies it"""
    from oracle import cport as O
    from oracle.keyswitch_ref import galois_coeff
    co = O.nwt_inverse_batch(x, qs, rps)
    co = np.stack([galois_coeff(co[j], k, qs[j]) for j in range(len(qs))])
    return O.nwt_forward_batch(co, qs, rps)


# ------------------------------------------------------------------------------------------------ a. accumulator families
def _edge_input(qs, rps, L, N, seed, hold=None):
    """[L][N] NTT domain: the transform of edge coefficients, the limbs ``hold`` (0 and L // 2 by default) at q - 1 in every NTT slot"""
    from oracle import cport as O
    coef = np.stack([KW.edge_coefficients(qs[l], [q for q in qs if q != qs[l]], N, seed) for l in range(L)])
    c = O.nwt_forward_batch(coef, qs[:L], rps[:L])
    for l in (0, L // 2) if hold is None else hold:
        c[l] = qs[l] - 1
    return c


def _same_sign_rows(x, q):
    """x: [terms][N] words != 0 of one limb -> key words that run a same-sign block in every slot (all q - 1 on the integer path).  With
    a whole fold block of FP64 terms the reach the design claims is asserted on these very words: >= 3.9 q before a fold."""
    path = "f64" if q < 1 << 50 else "u64"
    assert (x != 0).all()
    xinv = KW.inverse_words(x, q)
    y, reach = KW.same_sign_block(x, q, path, xinv=xinv)
    if path == "f64" and x.shape[0] >= 8:
        assert 3.9 * q <= reach[0] < 8 * q and reach[1] < 8 * q, (reach[0] / q, reach[1] / q)
    return y, xinv, path


def _family_key(x, qs):
    """[dnum][2][M][N]: half 0 = same-sign blocks over the digits (all q - 1 on the integer path), half 1 = the families in turn"""
    dnum, M, N = x.shape
    key = np.zeros((dnum, 2, M, N), dtype=U)
    turn = (np.arange(N)[None, :] + np.arange(dnum)[:, None]) % len(KW.FAMILIES)
    for j in range(M):
        q, xj = int(qs[j]), np.ascontiguousarray(x[:, j])
        key[:, 0, j], xinv, path = _same_sign_rows(xj, q)
        ys = KW.product_families(xj, q, path, xinv=xinv)
        ys = ys[0] if path == "f64" else ys
        for f, name in enumerate(KW.FAMILIES):
            key[:, 1, j] = np.where(turn == f, ys[name], key[:, 1, j])
    return key


FAMILY_SHAPES = [(10, 8, 1, 8, 50), (10, 9, 1, 9, 50), (10, 17, 1, 17, 50), (10, 9, 2, 9, 61), (10, 17, 2, 17, "mixed"), (13, 9, 2, 9, 50),
                 (13, 4, 2, 2, 50)]


@pytest.mark.parametrize("logn,L,K,dnum,kind", FAMILY_SHAPES)
def test_accumulator_families_through_apply_and_rotate(F, eng, logn, L, K, dnum, kind):
    from oracle.keyswitch_ref import keyswitch_ref, rotate_ref
    N = 1 << logn
    qs, rps, t, ks, ab = _plan(F, eng, logn, L, K, dnum, kind)
    c = _edge_input(qs, rps, L, N, logn + L)
    evk = _family_key(KW.extended_digits(c, qs, L, K, dnum, logn, rps), qs)
    want = keyswitch_ref(c, evk, qs, L, K, dnum, logn, rps=rps)
    dc, dk = eng.upload(c), eng.upload(evk)
    for fused in (0, 1):
        eng.set_option("ks_fused", fused)
        try:
            _eq(ks.apply(dc, dk), want, f"ks_fused {fused}")
        finally:
            eng.set_option("ks_fused", -1)
    o = ks.apply_checked(dc, dk, ab)
    _eq(o[:2], want, "apply_checked")
    _no_flag(o[2], "apply_checked")
    # rotation: the key switch's input is sigma(c1), so c1 = sigma^-1(c) meets the same key words
    k = 5
    c1 = _sigma(c, pow(k, -1, 2 * N), qs[:L], rps[:L])
    c0 = _edge_input(qs, rps, L, N, logn + L + 1)
    _eq(ks.rotate(eng.upload(c0), eng.upload(c1), k, dk), rotate_ref(c0, c1, k, evk, qs, L, K, dnum, logn), "rotate")
    eng.check()


@pytest.mark.parametrize("logn,L,K,dnum,kind", FAMILY_SHAPES)
def test_accumulator_families_through_hoisted_rotations(F, eng, logn, L, K, dnum, kind):
    """one to five elements: every k_ks_mac_multi<R> runs, and the fifth element starts a second group"""
    from oracle.keyswitch_ref import rotate_hoisted_ref
    N = 1 << logn
    qs, rps, t, ks, ab = _plan(F, eng, logn, L, K, dnum, kind)
    c1 = _edge_input(qs, rps, L, N, logn + L)
    c0 = _edge_input(qs, rps, L, N, logn + L + 1)
    x = KW.extended_digits(c1, qs, L, K, dnum, logn, rps)
    elts = [3, 5, 2 * N - 1, 9, (1 << (logn - 1)) + 1]
    # the inner product of element k multiplies sigma_k(x_d) with the key: the families are designed against those words
    keys = [_family_key(np.stack([_sigma(x[d], k, qs, rps) for d in range(dnum)]), qs) for k in elts]
    want = [rotate_hoisted_ref(c0, c1, k, key, qs, L, K, dnum, logn) for k, key in zip(elts, keys)]
    d0, d1 = eng.upload(c0), eng.upload(c1)
    prepared = [ks.prepare_galois_key(eng.upload(key), k) for k, key in zip(elts, keys)]
    for n in (1, 2, 3, 4, 5):
        outs = ks.rotate_hoisted(d0, d1, elts[:n], prepared[:n])
        for r in range(n):
            _eq(outs[r], want[r], f"{n} elements, element {r}")
    outs, flags = ks.rotate_hoisted_checked(d0, d1, elts, prepared, ab)
    for r in range(5):
        _eq(outs[r], want[r], f"checked, element {r}")
    _no_flag(flags, "rotate_hoisted_checked")
    eng.check()


# ------------------------------------------------------------------------------------------------ b. diagonal sums, tensor
@pytest.mark.parametrize("kind", [50, 61])
@pytest.mark.parametrize("n1", [8, 9, 17])
def test_diagonal_sums_run_same_sign_blocks(F, eng, n1, kind):
    """The inner sum of giant step g is sum_b diag[g][b] R_b over the baby rotations R_b, both parts sharing the diagonal word: the
    diagonals of g = 0 are solved against part 0 of the oracle's rotated parts, those of g = 1 against part 1, so that the n1 terms of
    every slot form same-sign blocks (all q - 1 on the integer path)."""
    from oracle.keyswitch_ref import bsgs_matvec_ref, rotate_hoisted_ref
    logn, L, K, dnum, n2 = 8, 2, 1, 2, 2
    N = 1 << logn
    qs, rps, t, ks, ab = _plan(F, eng, logn, L, K, dnum, kind)
    rng = np.random.default_rng(n1)
    c0, c1 = _edge_input(qs, rps, L, N, n1, hold=(0,)), _edge_input(qs, rps, L, N, n1 + 1, hold=(1,))
    key = lambda: np.stack([np.stack([np.stack([rng.integers(0, q, N, dtype=U) for q in qs]) for _ in range(2)]) for _ in range(dnum)])
    baby_elts = [pow(3, b, 2 * N) for b in range(1, n1)]
    giant_elts = [pow(3, g * n1, 2 * N) for g in range(1, n2)]
    baby_keys, giant_keys = [key() for _ in baby_elts], [key() for _ in giant_elts]
    R = [(c0, c1)] + [rotate_hoisted_ref(c0, c1, e, k, qs, L, K, dnum, logn) for e, k in zip(baby_elts, baby_keys)]
    diags = np.zeros((n2, n1, L, N), dtype=U)
    for g in range(n2):
        for l in range(L):
            diags[g, :, l] = _same_sign_rows(np.stack([R[b][g][l] for b in range(n1)]), int(qs[l]))[0]
    want = bsgs_matvec_ref(c0, c1, diags, baby_elts, baby_keys, giant_elts, giant_keys, qs, L, K, dnum, logn)
    d0, d1, dd = eng.upload(c0), eng.upload(c1), eng.upload(diags)
    prepared = [ks.prepare_galois_key(eng.upload(k), e) for k, e in zip(baby_keys, baby_elts)]
    d_giant = [eng.upload(k) for k in giant_keys]
    _eq(ks.bsgs_matvec(d0, d1, dd, n1, n2, baby_elts, prepared, giant_elts, d_giant), want, "bsgs_matvec")
    o = ks.bsgs_matvec_checked(d0, d1, dd, n1, n2, baby_elts, prepared, giant_elts, d_giant, ab)
    _eq(o[:2], want, "bsgs_matvec_checked")
    assert len(o[2]["giant"]) == n2 and len(o[2]["baby"]["rot"]) == n1 - 1
    _no_flag(o[2], "bsgs_matvec_checked")
    eng.check()


@pytest.mark.parametrize("logn,kind", [(8, 50), (8, 61), (13, "mixed")])
def test_tensor_cross_term_at_the_rounding_boundary_and_at_the_largest_operands(F, eng, logn, kind):
    from oracle.keyswitch_ref import tensor_ref
    N, L = 1 << logn, 4
    qs, rps, t, ks, ab = _plan(F, eng, logn, L, 1, L, kind)
    rng = np.random.default_rng(logn)
    a0, a1 = (np.stack([rng.integers(1, q, N, dtype=U) for q in qs[:L]]) for _ in range(2))
    b0, b1 = np.zeros_like(a0), np.zeros_like(a0)
    third = np.arange(N) % 3
    for l in range(L):
        q = qs[l]
        i0, i1 = KW.inverse_words(a0[l], q), KW.inverse_words(a1[l], q)
        lo, hi = np.full(N, (q - 1) // 2, dtype=U), np.full(N, (q + 1) // 2, dtype=U)
        # a0 b1 and a1 b0 both at (q - 1) / 2, both at (q + 1) / 2, and every operand at q - 1
        b1[l] = np.where(third == 0, KW.mul(i0, lo, q), KW.mul(i0, hi, q))
        b0[l] = np.where(third == 0, KW.mul(i1, lo, q), KW.mul(i1, hi, q))
        for v in (a0, a1, b0, b1):
            v[l, third == 2] = q - 1
    want = tensor_ref(a0, a1, b0, b1, qs)
    d = [eng.upload(v) for v in (a0, a1, b0, b1)]
    _eq(ks.tensor(*d), want, "tensor")
    o = ks.tensor_checked(*d)
    _eq(o[:3], want, "tensor_checked")
    _no_flag(o[3], "tensor_checked")
    eng.check()


# ------------------------------------------------------------------------------------------------ c. dictated accumulator
def _digit_input(qs, rps, L, K, dnum, N, seed):
    """[L][N] NTT domain whose coefficients are edge coefficients (one-limb digits) or worst-case digit columns over each digit's limbs"""
    from oracle import cport as O
    M, alpha = L + K, -(-L // dnum)
    coef = np.zeros((L, N), dtype=U)
    for d in range(dnum):
        lo, hi = d * alpha, min(L, (d + 1) * alpha)
        others = [qs[j] for j in range(M) if j < lo or j >= hi]
        coef[lo:hi] = KW.edge_coefficients(qs[lo], others, N, seed)[None] if hi - lo == 1 else KW.digit_columns(qs[lo:hi], others, N, seed)[0]
    return O.nwt_forward_batch(coef, qs[:L], rps[:L])


def _p_mod(qs, L):
    return [int(np.prod([int(p) % int(q) for p in qs[L:]], dtype=object)) % int(q) for q in qs[:L]]


def _dictated_key(x, qs, rps, L, K, N, seed, plain=0, out_rows=None, adds=(None, None)):
    """A key solved so that the special rows of acc are the transform of worst-case columns over the special base and the ciphertext
    rows put the tail on its edges (out_rows None: tail_targets, with addends to match) or make the tail's output row j of half h equal
    out_rows[h][j] given the addends ``adds``.  -> (key, addends [2][L][N])"""
    from oracle import cport as O
    Q, P = [int(q) for q in qs[:L]], [int(p) for p in qs[L:]]
    pm = _p_mod(qs, L)
    rng = np.random.default_rng(seed)
    y = np.stack([np.stack([np.stack([rng.integers(0, q, N, dtype=U) for q in qs]) for _ in range(2)]) for _ in range(x.shape[0])])
    target = np.zeros((2, L + K, N), dtype=U)
    addends = np.zeros((2, L, N), dtype=U)
    for h in range(2):
        cols = KW.digit_columns(P, Q, N, seed + h)[0] if K > 1 else KW.edge_coefficients(P[0], Q, N, seed + h)[None]
        tP = cols
        if plain:                                  # the oracle multiplies by t^-1 before it converts: the columns are what it converts
            tP = np.stack([KW.mul(cols[k], np.full(N, plain % P[k], dtype=U), P[k]) for k in range(K)])
        target[h, L:] = O.nwt_forward_batch(tP, P, rps[L:])
        conv = O.baseconv_exact(cols, P, Q)
        if plain:
            conv = np.stack([KW.mul(conv[j], np.full(N, plain % Q[j], dtype=U), Q[j]) for j in range(L)])
        cn = O.nwt_forward_batch(conv, Q, rps[:L])
        for j in range(L):
            pinv = pow(pm[j], -1, Q[j])
            if out_rows is None:
                target[h, j], addends[h, j] = KW.tail_targets(cn[j], Q[j], add=True, pinv=pinv, seed=seed + 7 * h + j)
            else:
                v = (out_rows[h][j] + (U(Q[j]) - adds[h][j])) % U(Q[j])          # the scaled word the tail must form
                target[h, j] = (cn[j] + KW.mul(v, np.full(N, pm[j], dtype=U), Q[j])) % U(Q[j])
                addends[h, j] = adds[h][j]
    key, undictated = KW.solve_key_for_acc(x, y, target, qs)
    assert undictated == 0
    return key, addends


DICTATED_SHAPES = [(10, 4, 2, 2, 50), (10, 4, 1, 4, 50), (12, 6, 3, 2, 61), (13, 4, 2, 2, 50), (13, 5, 3, 2, "mixed"), (14, 5, 2, 5, 50)]


@pytest.mark.parametrize("logn,L,K,dnum,kind", DICTATED_SHAPES)
def test_dictated_accumulator_through_mod_down_and_tail(F, eng, logn, L, K, dnum, kind):
    from oracle.keyswitch_ref import keyswitch_ref
    N = 1 << logn
    qs, rps, t, ks, ab = _plan(F, eng, logn, L, K, dnum, kind)
    c = _digit_input(qs, rps, L, K, dnum, N, logn + dnum)
    evk, (a0, a1) = _dictated_key(KW.extended_digits(c, qs, L, K, dnum, logn, rps), qs, rps, L, K, N, logn * 3 + K)
    plain = keyswitch_ref(c, evk, qs, L, K, dnum, logn, rps=rps)
    relin = keyswitch_ref(c, evk, qs, L, K, dnum, logn, add0=a0, add1=a1, rps=rps)
    one = keyswitch_ref(c, evk, qs, L, K, dnum, logn, add0=a0, rps=rps)
    dc, dk, d0, d1 = eng.upload(c), eng.upload(evk), eng.upload(a0), eng.upload(a1)
    for fused in (0, 1):
        eng.set_option("ks_fused", fused)
        try:
            _eq(ks.apply(dc, dk), plain, f"apply, ks_fused {fused}")
            _eq(ks.relinearize(d0, d1, dc, dk), relin, f"relinearize, ks_fused {fused}")
        finally:
            eng.set_option("ks_fused", -1)
    # rotation: one addend, sigma(c0); c0 = sigma^-1(addend), c1 = sigma^-1(c)
    k = 3
    kinv = pow(k, -1, 2 * N)
    r0, r1 = _sigma(a0, kinv, qs[:L], rps[:L]), _sigma(c, kinv, qs[:L], rps[:L])
    _eq(ks.rotate(eng.upload(r0), eng.upload(r1), k, dk), one, "rotate")
    o = ks.apply_checked(dc, dk, ab)
    _eq(o[:2], plain, "apply_checked")
    _no_flag(o[2], "apply_checked")
    o = ks.relinearize_checked(d0, d1, dc, dk, ab)
    _eq(o[:2], relin, "relinearize_checked")
    _no_flag(o[2], "relinearize_checked")
    eng.check()


def test_dictated_accumulator_with_a_plain_modulus(F, eng):
    from oracle.keyswitch_ref import keyswitch_ref
    logn, L, K, dnum, kind, tp = 11, 5, 2, 5, 50, 786433
    N = 1 << logn
    qs, rps, t, ks, ab = _plan(F, eng, logn, L, K, dnum, kind)
    c = _digit_input(qs, rps, L, K, dnum, N, 11)
    evk, (a0, a1) = _dictated_key(KW.extended_digits(c, qs, L, K, dnum, logn, rps), qs, rps, L, K, N, 35, plain=tp)
    dc, dk, d0, d1 = eng.upload(c), eng.upload(evk), eng.upload(a0), eng.upload(a1)
    ks.set_plain_modulus(tp)
    try:
        for fused in (0, 1):
            eng.set_option("ks_fused", fused)
            try:
                _eq(ks.apply(dc, dk), keyswitch_ref(c, evk, qs, L, K, dnum, logn, rps=rps, plain_modulus=tp), f"apply, ks_fused {fused}")
                _eq(ks.relinearize(d0, d1, dc, dk), keyswitch_ref(c, evk, qs, L, K, dnum, logn, add0=a0, add1=a1, rps=rps, plain_modulus=tp),
                    f"relinearize, ks_fused {fused}")
            finally:
                eng.set_option("ks_fused", -1)
    finally:
        ks.set_plain_modulus(0)
    eng.check()


# ------------------------------------------------------------------------------------------------ d. rescale, fused multiply
def _rescale_rows(qs, rps, L, N, seed):
    """[L][N] NTT domain: the last limb is the transform of edge coefficients against every remaining prime; limb j < L - 1 is
    NTT(delta_j) plus 0, q_j - 1 (the borrow by one), 1 ... in turn (tail_targets on delta's transform)"""
    from oracle import cport as O
    Q = [int(q) for q in qs[:L]]
    y = KW.edge_coefficients(Q[L - 1], Q[:L - 1], N, seed)
    out = np.zeros((L, N), dtype=U)
    out[L - 1] = O.nwt_forward(y, Q[L - 1], rps[L - 1])
    delta = np.stack([y % U(q) for q in Q[:L - 1]])
    dn = O.nwt_forward_batch(delta, Q[:L - 1], rps[:L - 1])
    for j in range(L - 1):
        out[j] = KW.tail_targets(dn[j], Q[j], pinv=pow(Q[L - 1] % Q[j], -1, Q[j]), seed=seed + j)[0]
    return out


RESCALE_BITS = [[50] * 5, [61] * 5, [50, 61, 50, 50, 61], [61, 50, 61, 50], [50, 50]]


@pytest.mark.parametrize("bits", RESCALE_BITS, ids=lambda b: "-".join(map(str, b)))
@pytest.mark.parametrize("logn", [10, 12, 13, 15])
def test_rescale_on_dictated_coefficients(F, eng, logn, bits):
    from oracle import cport as O
    from oracle.keyswitch_ref import rescale_ref
    N, L = 1 << logn, len(bits)
    qs = F.create_moduli(N, bits + [61])
    t = eng.tables(logn, qs)
    rps = np.stack([O.root_powers(q, logn) for q in qs])
    ks, ab = F.KeySwitch(eng, t, L, 1, L), F.Abft(eng, t)
    parts = np.stack([_rescale_rows(qs, rps, L, N, logn + 10 * p) for p in range(3)])
    want = rescale_ref(parts, qs, L, logn)
    # the dictated words are what the oracle's own steps see
    y = O.nwt_inverse(parts[0, L - 1], qs[L - 1], rps[L - 1])
    assert [int(v) for v in y[:3]] == [0, 1, qs[L - 1] - 1]
    dc = eng.upload(parts)
    for n in (1, 2, 3):
        got = ks.rescale(dc, n_parts=n).download().reshape(n, L - 1, N)
        assert (got == want[:n]).all(), f"{n} parts: first at {np.argwhere(got != want[:n])[0].tolist()}"
        o, fl = ks.rescale_checked(dc, ab, n_parts=n)
        assert (o.download().reshape(n, L - 1, N) == want[:n]).all(), f"checked, {n} parts"
        _no_flag(fl, f"rescale_checked, {n} parts")
    eng.check()


@pytest.mark.parametrize("logn,L,K,dnum,kind", [(13, 4, 2, 2, 50), (13, 5, 3, 2, "mixed")])
def test_hmult_with_a_solved_relinearisation_key(F, eng, logn, L, K, dnum, kind):
    """The tensor block is whatever the oracle says it is; the key is solved after it, so that the relinearised parts are
    _rescale_rows: the fused transform NTT(conv + P y) sees the mod-down's worst-case columns and the rescale's edges in one call"""
    from oracle.keyswitch_ref import hmult_ref, tensor_ref
    N = 1 << logn
    qs, rps, t, ks, ab = _plan(F, eng, logn, L, K, dnum, kind)
    ops = [_edge_input(qs, rps, L, N, logn + i) for i in range(4)]
    d0, d1, d2 = tensor_ref(*ops, qs)
    outs = [_rescale_rows(qs, rps, L, N, 50 + h) for h in range(2)]
    rlk, _ = _dictated_key(KW.extended_digits(d2, qs, L, K, dnum, logn, rps), qs, rps, L, K, N, logn + K, out_rows=outs, adds=(d0, d1))
    d, dk = [eng.upload(v) for v in ops], eng.upload(rlk)
    for rescale in (True, False):
        want = hmult_ref(*ops, rlk, qs, L, K, dnum, logn, rescale=rescale)
        if not rescale:
            assert (want[0] == outs[0]).all() and (want[1] == outs[1]).all()          # the relinearised parts are the dictated rows
        for fused in (1, 0):
            eng.set_option("hmult_fused_rescale", fused)
            try:
                _eq(ks.hmult(*d, dk, rescale=rescale), want, f"rescale {rescale}, hmult_fused_rescale {fused}")
            finally:
                eng.set_option("hmult_fused_rescale", 1)
        o = ks.hmult_checked(*d, dk, ab, rescale=rescale)
        _eq(o[:2], want, f"hmult_checked, rescale {rescale}")
        fl = dict(o[2])
        if not rescale:
            assert fl.pop("rescale") is None
        _no_flag(fl, f"hmult_checked, rescale {rescale}")
    eng.check()
