"""What the GPU tests of the stage-by-stage checked composites (key switch, rescale / multiply, hoisted rotations, BSGS product)
set up in the same way: the limb widths of a case and its moduli, tables, key-switch plan, detector and seeded generator."""
import numpy as np


def limb_bits(kind, L, K):
    """ciphertext limbs of one kind, special primes of the OTHER arithmetic path (mixed: alternating, specials alternating too)"""
    if kind == "50":
        return [50] * L + [61] * K
    if kind == "61":
        return [61] * L + [50] * K
    if kind == "50/50":
        return [50] * (L + K)
    if kind == "61/61":
        return [61] * (L + K)
    return [50 if i % 2 == 0 else 61 for i in range(L)] + [61 if i % 2 == 0 else 50 for i in range(K)]


def checked_plan(F, eng, logn, L, K, dnum, kind, seed):
    """(qs, tables, KeySwitch, Abft, rng): nothing is drawn from ``rng`` here, every test file draws its operands in its own order"""
    qs = F.create_moduli(1 << logn, limb_bits(kind, L, K))
    t = eng.tables(logn, qs)
    return qs, t, F.KeySwitch(eng, t, L, K, dnum), F.Abft(eng, t), np.random.default_rng(seed)
