"""The decryption-level properties of the composites, stated once over a backend: an object whose methods take and return numpy
residue arrays in the NTT domain ([limbs][N]).  tests/test_rlwe_helper.py runs them on the CPU oracle (OracleBackend below), where they
must hold and where deliberately wrong references must fail them; tests/test_gpu_decrypt_level.py runs the same functions on the engine.

Every property decrypts with helpers/rlwe.py and compares plaintexts: exactly modulo t over all N coefficients in the BGV form, within
the derived worst-case bounds of helpers/rlwe.py in the CKKS form.  Every bound is first asserted to leave the value below Q' / 2 of the
level it is checked at, otherwise the centred reconstruction would wrap and the comparison would mean nothing.  Each function returns
the number of coefficients it compared (N), so a caller can see that nothing was skipped.
"""
import numpy as np

from . import rlwe as R


def _amax(v):
    return max(abs(x) for x in v)


def prop_apply(p, be):
    """key switch of a uniform c from s^2 to s: out0 + out1 s - c s^2 is within the bound and, BGV, 0 modulo t"""
    c, key = p.uniform(), p.relin_key()
    o0, o1 = be.apply(c, key)
    assert p.b_ks < p.Q // 2
    err = R.keyswitch_error(o0, o1, c, p.s, p.s2, p.qs[:p.L])
    assert any(err), "a key switch without any error: the key was not used"
    return R.assert_error(err, p.b_ks, p.t, "key switch")


def prop_rotate(p, be, ct, m, k, hoisted=False):
    """decrypt(rotate_k(ct)) = sigma_k(m): exactly modulo t (BGV), the error within fresh + key-switch bound"""
    gk = p.galois_key(k)
    o0, o1 = (be.rotate_hoisted if hoisted else be.rotate)(ct[0], ct[1], k, gk)
    bound = R.noise_bound_rotate(p.b_fresh, p.b_ks)
    assert _amax(m) + bound < p.Q // 2
    dec, want = p.decrypt([o0, o1]), R.sigma_int(m, k)
    n = R.assert_error([d - w for d, w in zip(dec, want)], bound, p.t, f"rotation by {k}")
    if p.t:
        assert R.assert_plaintext(dec, want, p.t, f"rotation by {k}") == n
    return n


def prop_rescale(p, be, parts, m):
    """rescale / mod switch of 2 or 3 parts (3: decrypted with s^2): q_last dec' - v is within q_last * bound and, BGV, 0 modulo t, so that
    dec' = q_last^-1 m modulo t exactly; v is what the input decrypts to, m its plaintext"""
    n_parts, ql = len(parts), p.qs[p.L - 1]
    v = p.decrypt(parts)
    out = be.rescale(parts)
    assert len(out) == n_parts and all(o.shape == (p.L - 1, p.N) for o in out)
    assert _amax(v) // ql + R.noise_bound_rescale(p.N, n_parts, p.t) < p.Q // ql // 2
    dec = p.decrypt(list(out), p.L - 1)
    n = R.assert_rescaled(dec, v, ql, 0, n_parts, p.N, p.t, f"rescale of {n_parts} parts")
    if p.t:
        inv = pow(ql, -1, p.t)
        assert R.assert_plaintext(dec, [inv * x for x in m], p.t, f"mod switch of {n_parts} parts") == n
    return n


def prop_tensor(p, be, ct1, ct2, m1, m2):
    """three parts decrypt to v1 v2 over Z with no error added, hence to m1 m2 modulo (X^N + 1, t); returns (n, the three parts)"""
    d = be.tensor(ct1[0], ct1[1], ct2[0], ct2[1])
    v1, v2 = p.decrypt(ct1), p.decrypt(ct2)
    assert p.N * _amax(v1) * _amax(v2) < p.Q // 2
    dec, want = p.decrypt(list(d)), R.negacyclic_mul_int(v1, v2)
    bad = [i for i in range(p.N) if dec[i] != want[i]]
    assert not bad, f"tensor: the three parts do not decrypt to v1 v2 at {len(bad)} of {p.N} coefficients"
    mm = R.negacyclic_mul_int(m1, m2)
    if p.t:
        n = R.assert_plaintext(dec, mm, p.t, "tensor")
    else:
        n = R.assert_close(dec, mm, R.noise_bound_tensor(p.N, _amax(m1), _amax(m2), p.b_fresh, p.b_fresh), "tensor")
    return n, list(d)


def prop_hmult(p, be, ct1, ct2, m1, m2, rescale):
    """multiply, relinearise, optionally rescale: m1 m2 (BGV: modulo t, times q_last^-1 after the mod switch; CKKS: round(m1 m2 / q_last)
    within the bound after the rescale)"""
    o = be.hmult(ct1[0], ct1[1], ct2[0], ct2[1], p.relin_key(), rescale)
    mm = R.negacyclic_mul_int(m1, m2)
    a1, a2, ql = _amax(m1), _amax(m2), p.qs[p.L - 1]
    if not rescale:
        bound = R.noise_bound_hmult(p.N, a1, a2, p.b_fresh, p.b_fresh, p.b_ks)
        assert p.N * a1 * a2 + bound < p.Q // 2
        dec = p.decrypt(list(o))
        n = R.assert_error([d - w for d, w in zip(dec, mm)], bound, p.t, "multiply")
        if p.t:
            assert R.assert_plaintext(dec, mm, p.t, "multiply") == n
        return n
    bound = R.noise_bound_hmult(p.N, a1, a2, p.b_fresh, p.b_fresh, p.b_ks, ql, p.t)       # on q_last dec' - m1 m2
    assert (p.N * a1 * a2 + bound) // ql + 1 < p.Q // ql // 2
    dec = p.decrypt(list(o), p.L - 1)
    n = R.assert_error([ql * d - w for d, w in zip(dec, mm)], bound, p.t, "multiply and rescale")
    if p.t:
        inv = pow(ql, -1, p.t)
        assert R.assert_plaintext(dec, [inv * x for x in mm], p.t, "multiply and mod switch") == n
    else:
        assert R.assert_close(dec, [R.div_round(x, ql) for x in mm], -(-bound // ql) + 1, "multiply and rescale") == n
    return n


def bsgs_case(p, n1, n2, diag_below=1 << 10):
    """diagonals (integer coefficient polynomials with entries below diag_below, and their NTT forms [n2][n1][L][N]), Galois elements, keys"""
    Q = p.qs[:p.L]
    di = [[p.message(diag_below) for _ in range(n1)] for _ in range(n2)]
    diags = np.stack([np.stack([R.to_ntt(di[g][b], Q) for b in range(n1)]) for g in range(n2)])
    baby = [pow(3, b, 2 * p.N) for b in range(1, n1)]
    giant = [pow(3, g * n1, 2 * p.N) for g in range(1, n2)]
    return di, diags, baby, [p.galois_key(k) for k in baby], giant, [p.galois_key(k) for k in giant]


def prop_bsgs(p, be, ct, m, n1, n2, diag_below=1 << 10):
    """decrypt(bsgs_matvec(ct)) = sum_g sigma_G(sum_b diag[g][b] sigma_B(m)) over Z within the bound (CKKS form, a real encryption)"""
    assert p.t == 0
    assert np.asarray(ct[1]).any()
    di, diags, baby, baby_keys, giant, giant_keys = bsgs_case(p, n1, n2, diag_below)
    o0, o1 = be.bsgs_matvec(ct[0], ct[1], diags, n1, n2, baby, baby_keys, giant, giant_keys)
    want = [0] * p.N
    for g in range(n2):
        inner = [0] * p.N
        for b in range(n1):
            term = R.negacyclic_mul_int(di[g][b], m if b == 0 else R.sigma_int(m, baby[b - 1]))
            inner = [x + y for x, y in zip(inner, term)]
        if g:
            inner = R.sigma_int(inner, giant[g - 1])
        want = [x + y for x, y in zip(want, inner)]
    bound = R.noise_bound_bsgs(p.N, n1, n2, diag_below, p.b_fresh, p.b_ks)
    assert _amax(want) + bound < p.Q // 2 and bound < _amax(want) >> 8          # the bound is far below the value: the check has teeth
    return R.assert_close(p.decrypt([o0, o1]), want, bound, "BSGS product")


class OracleBackend:
    """the CPU restatement of the composites (oracle/keyswitch_ref.py) behind the backend interface; ks_t / rs_t: the plain modulus handed
    to the key switches / to the rescale (both the party's t unless a negative control says otherwise)"""

    def __init__(self, p, ks_t=None, rs_t=None, hmult_ref=False):
        self.p, self.ks_t, self.rs_t = p, (p.t if ks_t is None else ks_t), (p.t if rs_t is None else rs_t)
        self.use_hmult_ref = hmult_ref
        self.a = (p.qs, p.L, p.K, p.dnum, p.logn)

    def _sigma(self, x, k):
        from oracle.keyswitch_ref import galois_coeff
        Q = self.p.qs[:self.p.L]
        co = R.intt(x, Q)
        return R.ntt(np.stack([galois_coeff(co[l], k, Q[l]) for l in range(len(Q))]), Q)

    def apply(self, c, key):
        from oracle.keyswitch_ref import keyswitch_ref
        return keyswitch_ref(c, key, *self.a, plain_modulus=self.ks_t)

    def rotate(self, c0, c1, k, gk):
        from oracle.keyswitch_ref import keyswitch_ref, rotate_ref
        if not self.ks_t:
            return rotate_ref(c0, c1, k, gk, *self.a)
        return keyswitch_ref(self._sigma(c1, k), gk, *self.a, add0=self._sigma(c0, k), plain_modulus=self.ks_t)

    def rotate_hoisted(self, c0, c1, k, gk):
        from oracle.keyswitch_ref import keyswitch_ref, rotate_hoisted_ref
        if not self.ks_t:
            return rotate_hoisted_ref(c0, c1, k, gk, *self.a)
        return keyswitch_ref(c1, gk, *self.a, add0=self._sigma(c0, k), plain_modulus=self.ks_t, sigma_ext=k)

    def rescale(self, parts):
        from oracle.keyswitch_ref import rescale_ref
        return list(rescale_ref(parts, self.p.qs, self.p.L, self.p.logn, plain_modulus=self.rs_t))

    def tensor(self, a0, a1, b0, b1):
        from oracle.keyswitch_ref import tensor_ref
        return tensor_ref(a0, a1, b0, b1, self.p.qs)

    def hmult(self, a0, a1, b0, b1, rlk, rescale):
        from oracle.keyswitch_ref import hmult_ref, keyswitch_ref
        if self.use_hmult_ref:
            return hmult_ref(a0, a1, b0, b1, rlk, *self.a, rescale=rescale, plain_modulus=self.rs_t)
        d0, d1, d2 = self.tensor(a0, a1, b0, b1)
        c = keyswitch_ref(d2, rlk, *self.a, add0=d0, add1=d1, plain_modulus=self.ks_t)
        return self.rescale(list(c)) if rescale else c

    def bsgs_matvec(self, c0, c1, diags, n1, n2, baby, baby_keys, giant, giant_keys):
        from oracle.keyswitch_ref import bsgs_matvec_ref
        return bsgs_matvec_ref(c0, c1, diags, baby, baby_keys, giant, giant_keys, *self.a)
