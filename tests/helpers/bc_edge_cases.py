"""Inputs of the base-conversion edge tests, shared by tests/test_gpu_baseconv_edges.py and the child process it starts
(tests/helpers/bc_variant0_child.py): both build the same words from the same seeds, so the child only has to report a hash."""
import hashlib

import numpy as np

from helpers import bc_worst_case as W

N_SMALL = 300                     # two workgroups, the second partial
N_LONG = (1 << 22) + 3            # past 16384 workgroups of 256: a second trip through the coefficient loop
KS = (1, 3, 6, 8, 13)
VARIANT0_SIZES = (1, 4, 5, 8, 9, 12, 13, 16)
VARIANT0_K = 6


def moduli(F, m, k, big):
    """m + k distinct primes: all 50 bits (FP64 plan), or with one 61-bit prime among the inputs (integer plan); the rule of
    tests/test_gpu_baseconv_checked.py"""
    qs = F.create_moduli(1 << 10, [50] * (m + k - 1) + [61 if big else 50])
    qs = qs[-1:] + qs[:-1] if big else qs
    return qs[:m], qs[m:]


def columns(mi, mo, N, seed):
    """-> x [m][N] (columns 0 .. n_w - 1 the worst columns, the rest random), names of the worst columns, their expected words [k][n_w]
    from Python integers"""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.integers(0, p, N, dtype=np.uint64) for p in mi])
    names, res, want = W.worst_residues(mi, mo)
    assert len(names) <= N
    x[:, :len(names)] = np.array(res, dtype=np.uint64).T
    return x, names, np.array(want, dtype=np.uint64).T.reshape(len(mo), len(names))


def small_case(F, m, k, big):
    mi, mo = moduli(F, m, k, big)
    return (mi, mo) + columns(mi, mo, N_SMALL, (m * 64 + k) * 2 + big)


def long_case(F):
    """-> mi, mo, x, names, expected words of the worst columns, the columns to compare"""
    mi, mo = moduli(F, 2, 1, False)
    x, names, want = columns(mi, mo, N_LONG, 22)
    sample = np.random.default_rng(23).integers(0, N_LONG, 4096)
    cols = np.unique(np.concatenate([np.arange(8), np.arange(N_LONG - 8, N_LONG), sample]))
    return mi, mo, x, names, want, cols


def sha(words):
    return hashlib.sha256(np.ascontiguousarray(words, dtype=np.uint64).astype("<u8").tobytes()).hexdigest()


def convert(F, eng, mi, mo, x):
    """the plain call -> [k][N]"""
    N = x.shape[1]
    bc = F.BaseConv(eng, mi, mo)
    d_in, d_out = eng.upload(x), eng.alloc(len(mo) * N)
    bc.exact(d_out, d_in, N)
    return d_out.download().reshape(len(mo), N)
