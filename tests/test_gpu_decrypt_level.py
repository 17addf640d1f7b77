"""The composites at the DECRYPTION level on the GPU: the result of each unchecked call is decrypted with tests/helpers/rlwe.py (Python
integers, nothing of the engine) and compared with the plaintext the operation is defined to give -- exactly modulo t over all N
coefficients on plans with a plain modulus (the BGV form), within derived worst-case bounds in the CKKS form.  The word-for-word tests
compare the engine with oracle/keyswitch_ref.py, which restates the same sequence of steps; a mistake in the sequence itself would be
made on both sides.  These tests share nothing with that sequence (tests/helpers/decrypt_props.py; the same properties hold for the
oracle and reject wrong references in tests/test_rlwe_helper.py).

Plans, the smallest at which each route is still taken:
  A = 2^10, L 4, K 2, dnum 2, all 50-bit       one-launch transforms, two-limb digits
  B = 2^13, L 3, K 1, dnum 3, [50, 61, 50, 50]  the smallest two-launch size, one-limb conversions, the integer path beside the FP64 one
  C = 2^13, L 4, K 2, dnum 2, all 50-bit       the smallest shape on the fused-rescale route of hmult
BGV form: A and B with t in {65537, 786433}.  CKKS form: A and C.

fhe_rotate_hoisted honours the plain modulus (the special limbs are scaled by t^-1 after their INTT and the converted limbs by t, as in
the plain mod-down), so a BGV hoisted rotation is held to the same property as fhe_rotate.

CKKS multiply with rescale: messages below 2^25 keep the product far below Q, but m1 m2 / q_last is then no larger than the bound itself
(N 2^50 / 2^50 against N + 2), so the same property is also asserted on messages below 2^45, where the value (about 2^40 N) is far above
the bound, and on the multiply without rescale, where m1 m2 stands against the key-switch bound alone.

Every parametrised case counts itself in RAN; the last test of the module asserts that none was skipped."""
import collections

import numpy as np
import pytest

from helpers import decrypt_props as DP
from helpers import rlwe as R

pytestmark = pytest.mark.gpu

PLANS = {"A": (10, 4, 2, 2, [50] * 6), "B": (13, 3, 1, 3, [50, 61, 50, 50]), "C": (13, 4, 2, 2, [50] * 6)}
BGV = [("A", 65537), ("A", 786433), ("B", 65537), ("B", 786433)]
RAN = collections.Counter()


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


class EngineBackend:
    """KeySwitch's unchecked calls behind the backend interface of helpers/decrypt_props.py: numpy in, numpy out"""

    def __init__(self, F, eng, p, tables):
        self.F, self.eng, self.p, self.tables = F, eng, p, tables
        self.ks = F.KeySwitch(eng, tables, p.L, p.K, p.dnum)
        if p.t:
            self.ks.set_plain_modulus(p.t)

    def _up(self, *xs):
        return [self.eng.upload(np.ascontiguousarray(x)) for x in xs]

    @staticmethod
    def _down(outs):
        return tuple(o.download() for o in outs)

    def apply(self, c, key):
        return self._down(self.ks.apply(*self._up(c, key)))

    def rotate(self, c0, c1, k, gk):
        d0, d1, dk = self._up(c0, c1, gk)
        return self._down(self.ks.rotate(d0, d1, k, dk))

    def rotate_hoisted(self, c0, c1, k, gk):
        d0, d1, dk = self._up(c0, c1, gk)
        (o0, o1), = self.ks.rotate_hoisted(d0, d1, [k], [self.ks.prepare_galois_key(dk, k)])
        return self._down((o0, o1))

    def rescale(self, parts):
        d, = self._up(np.stack(parts))
        return list(self.ks.rescale(d, n_parts=len(parts)).download())

    def tensor(self, a0, a1, b0, b1):
        return self._down(self.ks.tensor(*self._up(a0, a1, b0, b1)))

    def hmult(self, a0, a1, b0, b1, rlk, rescale):
        return self._down(self.ks.hmult(*self._up(a0, a1, b0, b1, rlk), rescale=rescale))

    def bsgs_matvec(self, c0, c1, diags, n1, n2, baby, baby_keys, giant, giant_keys):
        d0, d1, dd = self._up(c0, c1, diags)
        prepared = [self.ks.prepare_galois_key(self._up(k)[0], e) for k, e in zip(baby_keys, baby)]
        return self._down(self.ks.bsgs_matvec(d0, d1, dd, n1, n2, baby, prepared, giant, self._up(*giant_keys)))


class CheckedBackend(EngineBackend):
    """hmult through the guarded call of the form (bgv_hmult_checked on a plan with a plain modulus, hmult_checked without)"""

    def hmult(self, a0, a1, b0, b1, rlk, rescale):
        call = self.ks.bgv_hmult_checked if self.p.t else self.ks.hmult_checked
        o0, o1, flags = call(*self._up(a0, a1, b0, b1, rlk), self.F.Abft(self.eng, self.tables), rescale=rescale)
        assert not flags["tensor"].any() and not any(f.any() for f in flags["keyswitch"].values())
        assert (flags["rescale"] is None) == (not rescale) and not (rescale and any(f.any() for f in flags["rescale"].values()))
        return self._down((o0, o1))


@pytest.fixture(scope="module")
def world(F, eng):
    """(party, backend) of a (plan, t), made once: secret, two messages and their encryptions; keys on demand, kept by the party"""
    made = {}

    def get(name, t):
        if (name, t) not in made:
            logn, L, K, dnum, bits = PLANS[name]
            N = 1 << logn
            qs = F.create_moduli(N, bits)
            assert [q.bit_length() for q in qs] == bits
            p = R.Party(N, qs, L, K, dnum, t, seed=logn * 1000003 + t)
            p.m1, p.m2 = p.message(t or 1 << 25), p.message(t or 1 << 25)
            p.ct1, p.ct2 = p.encrypt(p.m1), p.encrypt(p.m2)
            assert p.ct1[1].any() and p.ct2[1].any()
            made[name, t] = p, EngineBackend(F, eng, p, eng.tables(logn, qs))
        return made[name, t]
    return get


@pytest.mark.parametrize("name,t", BGV)
def test_bgv_key_switch_adds_a_bounded_multiple_of_t(eng, world, name, t):
    p, be = world(name, t)
    assert DP.prop_apply(p, be) == p.N
    eng.check()
    RAN["apply"] += 1


@pytest.mark.parametrize("k", [5, -1])
@pytest.mark.parametrize("name,t", BGV)
def test_bgv_rotation_decrypts_to_sigma_of_the_plaintext(eng, world, name, t, k):
    p, be = world(name, t)
    assert DP.prop_rotate(p, be, p.ct1, p.m1, k % (2 * p.N)) == p.N
    eng.check()
    RAN["rotate"] += 1


@pytest.mark.parametrize("name,t", [("A", 65537), ("B", 786433)])
def test_bgv_hoisted_rotation_decrypts_to_sigma_of_the_plaintext(eng, world, name, t):
    p, be = world(name, t)
    assert DP.prop_rotate(p, be, p.ct2, p.m2, 5, hoisted=True) == p.N
    eng.check()
    RAN["hoisted"] += 1


@pytest.mark.parametrize("name,t", BGV)
def test_bgv_tensor_and_mod_switch_of_two_and_three_parts(eng, world, name, t):
    """the three parts of the tensor product decrypt (with s^2) to m1 m2 modulo (X^N + 1, t); the mod switch of two parts and of those three
    gives q_last^-1 times the plaintext modulo t, over Q / q_last"""
    p, be = world(name, t)
    n, d = DP.prop_tensor(p, be, p.ct1, p.ct2, p.m1, p.m2)
    assert n == p.N
    assert DP.prop_rescale(p, be, list(p.ct1), p.m1) == p.N
    assert DP.prop_rescale(p, be, d, R.negacyclic_mul_int(p.m1, p.m2)) == p.N
    eng.check()
    RAN["tensor, mod switch"] += 1


@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("name,t", BGV)
def test_bgv_multiply_decrypts_to_the_product(eng, world, name, t, rescale):
    p, be = world(name, t)
    assert DP.prop_hmult(p, be, p.ct1, p.ct2, p.m1, p.m2, rescale) == p.N
    eng.check()
    RAN["bgv hmult"] += 1


@pytest.mark.parametrize("below", [25, 45])
@pytest.mark.parametrize("name,fused", [("A", 1), ("C", 1), ("C", 0)])
def test_ckks_multiply_with_rescale_decrypts_to_the_rounded_product(eng, world, name, fused, below):
    """plan C takes the fused-rescale route (mod-down and rescale behind one forward transform) unless hmult_fused_rescale is 0: both routes
    are decrypted; plan A is below the route's sizes"""
    p, be = world(name, 0)
    if below == 25:
        m1, m2, c1, c2 = p.m1, p.m2, p.ct1, p.ct2
    else:
        m1, m2 = p.message(1 << below), p.message(1 << below)
        c1, c2 = p.encrypt(m1), p.encrypt(m2)
    eng.set_option("hmult_fused_rescale", fused)
    try:
        assert DP.prop_hmult(p, be, c1, c2, m1, m2, True) == p.N
        assert DP.prop_hmult(p, be, c1, c2, m1, m2, False) == p.N
    finally:
        eng.set_option("hmult_fused_rescale", 1)
    eng.check()
    RAN["ckks hmult"] += 1


def test_ckks_bsgs_product_on_a_real_encryption(eng, world):
    p, be = world("A", 0)
    m = p.message(1 << 30)
    assert DP.prop_bsgs(p, be, p.encrypt(m), m, 2, 2) == p.N
    eng.check()
    RAN["bsgs"] += 1


@pytest.mark.parametrize("t", [65537, 0])
def test_guarded_multiply_decrypts_to_the_same_plaintext(F, eng, world, t):
    """one transitive check per form: the outputs of bgv_hmult_checked (hmult_checked without a plain modulus) at plan A, with no flag raised"""
    p, be = world("A", t)
    guarded = CheckedBackend(F, eng, p, be.tables)
    for rescale in (False, True):
        assert DP.prop_hmult(p, guarded, p.ct1, p.ct2, p.m1, p.m2, rescale) == p.N
    eng.check()
    RAN["guarded"] += 1


def test_no_case_was_skipped():
    """runs last, after the whole module"""
    n = dict(RAN)
    assert n == {"apply": 4, "rotate": 8, "hoisted": 2, "tensor, mod switch": 4, "bgv hmult": 8, "ckks hmult": 6, "bsgs": 1, "guarded": 2}
