"""tests/helpers/rlwe.py and tests/helpers/decrypt_props.py without a GPU: the toolkit round-trips, the CPU oracle's composites satisfy
every decryption-level property at plan A = (2^10, L 4, K 2, dnum 2, all 50-bit) in both forms, and the properties have teeth: reference
code that is wrong for a BGV plan fails them for the stated reason.  Nothing faulty runs on a GPU; the controls are CPU reference code."""
import random

import numpy as np
import pytest

from helpers import decrypt_props as DP
from helpers import rlwe as R
from oracle import cport as O

LOGN, L, K, DNUM = 10, 4, 2, 2
N = 1 << LOGN
FORMS = [0, 65537, 786433]


@pytest.fixture(scope="module")
def parties():
    qs = O.gen_primes(N, 50, L + K)
    made = {}

    def get(t):
        if t not in made:
            p = R.Party(N, qs, L, K, DNUM, t, seed=1000 + t)
            p.m1, p.m2 = p.message(t or 1 << 25), p.message(t or 1 << 25)
            p.ct1, p.ct2 = p.encrypt(p.m1), p.encrypt(p.m2)
            made[t] = p
        return made[t]
    return get


def test_integer_helpers_against_schoolbook():
    from oracle.keyswitch_ref import galois_coeff
    rnd = random.Random(3)
    n = 32
    a = [rnd.randrange(-(1 << 70), 1 << 70) for _ in range(n)]
    b = [rnd.randrange(-(1 << 40), 1 << 40) for _ in range(n)]
    want = [0] * n
    for i in range(n):
        for j in range(n):
            if i + j < n:
                want[i + j] += a[i] * b[j]
            else:
                want[i + j - n] -= a[i] * b[j]
    assert R.negacyclic_mul_int(a, b) == want
    assert R.negacyclic_mul_int(a, b, 786433) == [x % 786433 for x in want]
    assert R.negacyclic_mul_int(a, [0] * n) == [0] * n
    q = 65537
    for k in (3, 5, 2 * n - 1):
        pos = [x % q for x in a]
        assert [x % q for x in R.sigma_int(pos, k)] == [int(x) for x in galois_coeff(np.array(pos, dtype=np.uint64), k, q)]
        # sigma is a ring automorphism
        assert R.sigma_int(want, k) == R.negacyclic_mul_int(R.sigma_int(a, k), R.sigma_int(b, k))
    assert [R.centred(x, 7) for x in range(-7, 8)] == [0, 1, 2, 3, -3, -2, -1, 0, 1, 2, 3, -3, -2, -1, 0]
    assert [R.div_round(x, 10) for x in (-15, -14, -5, -4, 0, 4, 5, 14, 15)] == [-2, -1, -1, 0, 0, 0, 1, 1, 2]
    # CRT of residues gives back centred values
    qs = O.gen_primes(n, 50, 3)
    assert R.crt_centred(R.residues(a, qs), qs) == a


@pytest.mark.parametrize("t", FORMS)
def test_fresh_encryptions_round_trip(parties, t):
    p = parties(t)
    for m, ct in ((p.m1, p.ct1), (p.m2, p.ct2)):
        assert ct[1].any() and (ct[0] < np.array(p.qs[:L], dtype=np.uint64)[:, None]).all()
        dec = p.decrypt(ct)
        err = [d - x for d, x in zip(dec, m)]
        assert any(err)
        assert R.assert_error(err, R.noise_bound_fresh(t), t, "fresh encryption") == N
        if t:
            assert R.assert_plaintext(dec, m, t) == N and [d % t for d in dec] == m
    # a key of the stated shape: b + a s = E + P Qhat_d [Qhat_d^-1]_{Q_d} s_from over all L + K primes
    key = p.relin_key()
    assert key.shape == (DNUM, 2, L + K, N)
    Q, P = R.prod(p.qs[:L]), R.prod(p.qs[L:])
    for d in range(DNUM):
        Qd = R.prod(p.qs[d * 2:d * 2 + 2])
        factor = P * (Q // Qd) * pow(Q // Qd, -1, Qd)
        body = R.decrypt([key[d, 0], key[d, 1]], p.s, p.qs)
        e = [R.centred(x - factor * y, Q * P) for x, y in zip(body, p.s2)]
        assert R.assert_error(e, R.noise_bound_fresh(t), t, "key error") == N and any(e)


@pytest.mark.parametrize("t", FORMS)
def test_oracle_key_switch_and_rotations_hold_the_properties(parties, t):
    p = parties(t)
    be = DP.OracleBackend(p)
    assert DP.prop_apply(p, be) == N
    for k in (5, 2 * N - 1):
        assert DP.prop_rotate(p, be, p.ct1, p.m1, k) == N
    assert DP.prop_rotate(p, be, p.ct2, p.m2, 5, hoisted=True) == N


@pytest.mark.parametrize("t", FORMS)
def test_oracle_rescale_tensor_and_multiply_hold_the_properties(parties, t):
    p = parties(t)
    be = DP.OracleBackend(p)
    n, d = DP.prop_tensor(p, be, p.ct1, p.ct2, p.m1, p.m2)
    assert n == N
    mm = R.negacyclic_mul_int(p.m1, p.m2)
    if t:
        assert DP.prop_rescale(p, be, list(p.ct1), p.m1) == N
        assert DP.prop_rescale(p, be, d, mm) == N
    else:
        # CKKS: values wide enough that what is left after the division by q_last is far above the bound
        wide = p.message(1 << 90)
        assert DP.prop_rescale(p, be, list(p.encrypt(wide)), wide) == N
        w1, w2 = p.message(1 << 45), p.message(1 << 45)
        c1, c2 = p.encrypt(w1), p.encrypt(w2)
        assert DP.prop_rescale(p, be, DP.prop_tensor(p, be, c1, c2, w1, w2)[1], None) == N
        for resc in (False, True):
            assert DP.prop_hmult(p, be, c1, c2, w1, w2, resc) == N
    for resc in (False, True):
        assert DP.prop_hmult(p, be, p.ct1, p.ct2, p.m1, p.m2, resc) == N


def test_oracle_bsgs_product_holds_the_property(parties):
    p = parties(0)
    m = p.message(1 << 30)
    assert DP.prop_bsgs(p, DP.OracleBackend(p), p.encrypt(m), m, 2, 2) == N


def test_hmult_ref_is_the_chain_in_the_ckks_form_only(parties):
    """hmult_ref hands its plain modulus to the rescale only: the chain's words without one, other words with one"""
    from oracle.keyswitch_ref import hmult_ref
    for t in (0, 65537):
        p = parties(t)
        a = (p.ct1[0], p.ct1[1], p.ct2[0], p.ct2[1], p.relin_key())
        h = hmult_ref(*a, p.qs, L, K, DNUM, LOGN, plain_modulus=t)
        w = DP.OracleBackend(p).hmult(*a, True)
        assert bool((h[0] == w[0]).all() and (h[1] == w[1]).all()) == (t == 0)


@pytest.mark.parametrize("t", [65537, 786433])
def test_a_ckks_key_switch_on_a_bgv_ciphertext_fails_the_property(parties, t):
    p = parties(t)
    wrong = DP.OracleBackend(p, ks_t=0)
    with pytest.raises(AssertionError, match="key switch: not 0 modulo t"):
        DP.prop_apply(p, wrong)
    with pytest.raises(AssertionError, match="rotation by 5: not 0 modulo t"):
        DP.prop_rotate(p, wrong, p.ct1, p.m1, 5)


@pytest.mark.parametrize("t", [65537, 786433])
def test_a_ckks_rescale_on_a_bgv_ciphertext_fails_the_property(parties, t):
    p = parties(t)
    wrong = DP.OracleBackend(p, rs_t=0)
    with pytest.raises(AssertionError, match="rescale of 2 parts: not 0 modulo t"):
        DP.prop_rescale(p, wrong, list(p.ct1), p.m1)
    d = DP.OracleBackend(p).tensor(*p.ct1, *p.ct2)
    with pytest.raises(AssertionError, match="rescale of 3 parts: not 0 modulo t"):
        DP.prop_rescale(p, wrong, list(d), R.negacyclic_mul_int(p.m1, p.m2))


@pytest.mark.parametrize("t", [65537, 786433])
def test_hmult_ref_with_a_plain_modulus_fails_the_product_property(parties, t):
    """the composite that tests/test_gpu_bgv_checked.py declines as its reference: relinearised in the CKKS form, it is not a BGV multiply"""
    p = parties(t)
    wrong = DP.OracleBackend(p, hmult_ref=True)
    with pytest.raises(AssertionError, match="multiply: not 0 modulo t"):
        DP.prop_hmult(p, wrong, p.ct1, p.ct2, p.m1, p.m2, False)
    with pytest.raises(AssertionError, match="multiply and rescale: not 0 modulo t"):
        DP.prop_hmult(p, wrong, p.ct1, p.ct2, p.m1, p.m2, True)


def test_the_bounds_reject_what_they_should(parties):
    """a bound one below the worst coefficient raises; a plaintext off by one at ONE coefficient raises"""
    p = parties(65537)
    dec = p.decrypt(p.ct1)
    err = [d - x for d, x in zip(dec, p.m1)]
    with pytest.raises(AssertionError, match="above the bound"):
        R.assert_error(err, max(abs(x) for x in err) - 1, p.t)
    off = list(p.m1)
    off[N - 1] += 1
    with pytest.raises(AssertionError, match="at 1 of 1024 coefficients"):
        R.assert_plaintext(dec, off, p.t)
    with pytest.raises(AssertionError, match="off by"):
        R.assert_close(dec, [d + 5 for d in dec], 4)
