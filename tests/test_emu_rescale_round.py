"""The shared per-word step of the round-to-nearest rescale (csrc/rescale_round.hpp), built for the CPU, against Python integers:
r = y if y <= h else y - q, and the step returns r mod q_j -- for every size relation of the two primes (q > q_j, q < q_j,
q >= 2 q_j down to 30-bit q_j under a 61-bit q), as a canonical word and through both arithmetic paths."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers.emu_build import build_emu
from oracle import cport as O

U = np.uint64
N_RING = 1 << 10


@pytest.fixture(scope="module")
def emu():
    lib = build_emu("libemu_rescale_round.so", ["emu_rescale_round.cpp"], ["rescale_round.hpp", "modarith.hpp"])
    p64 = C.POINTER(C.c_uint64)
    lib.emu_round_residue.restype = None
    lib.emu_round_residue.argtypes = [p64, C.c_size_t, C.c_uint64, C.c_uint64, p64]
    lib.emu_round_residue_path.restype = C.c_int
    lib.emu_round_residue_path.argtypes = [p64, C.c_size_t, C.c_uint64, C.c_uint64, C.c_int, p64]
    return lib


NAMES = ["50>50", "50<50", "61>61", "61<61", "61 last, 50", "50 last, 61", "61 last, 30"]


@functools.lru_cache(maxsize=None)
def _pairs():
    p50, p61, p30 = O.gen_primes(N_RING, 50, 2), O.gen_primes(N_RING, 61, 2), O.gen_primes(N_RING, 30, 1)
    lo50, hi50 = sorted(p50)
    lo61, hi61 = sorted(p61)
    return {"50>50": (hi50, lo50), "50<50": (lo50, hi50), "61>61": (hi61, lo61), "61<61": (lo61, hi61), "61 last, 50": (hi61, hi50),
            "50 last, 61": (hi50, hi61), "61 last, 30": (hi61, p30[0])}



def _words(q, seed):
    h = (q - 1) // 2
    edge = [0, 1, h - 1, h, h + 1, q - 2, q - 1]
    rng = np.random.default_rng(seed)
    return np.concatenate([np.array(edge, dtype=U), rng.integers(0, q, 4096, dtype=U)])


def _want(y, q, qj):
    h = (q - 1) // 2
    return np.array([(int(v) if int(v) <= h else int(v) - q) % qj for v in y], dtype=U)


def _ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


@pytest.mark.parametrize("name", NAMES)
def test_round_residue_against_python_integers(emu, name):
    q, qj = _pairs()[name]
    assert q % 2 == 1
    if name == "61 last, 30":
        assert q >= 2 * qj
    y = _words(q, seed=len(name))
    want = _want(y, q, qj)
    got = np.zeros_like(y)
    emu.emu_round_residue(_ptr(y), y.size, q, qj, _ptr(got))
    assert (got == want).all(), np.argwhere(got != want)[:4].tolist()
    assert (got < U(qj)).all()
    # the SEAL sequence gives the same residues: ((y + h mod q) mod q_j - h mod q_j) mod q_j
    h = (q - 1) // 2
    seal = np.array([(((int(v) + h) % q) % qj - h % qj) % qj for v in y[:64]], dtype=U)
    assert (seal == want[:64]).all()
    for path in ((0, 1) if qj < 1 << 50 else (1,)):
        thru = np.zeros_like(y)
        assert emu.emu_round_residue_path(_ptr(y), y.size, q, qj, path, _ptr(thru)) == 0
        assert (thru == want).all(), (path, np.argwhere(thru != want)[:4].tolist())


def test_fp64_path_refuses_a_limb_outside_it(emu):
    q, qj = _pairs()["50 last, 61"]
    y = _words(q, 0)
    out = np.zeros_like(y)
    assert emu.emu_round_residue_path(_ptr(y), y.size, q, qj, 0, _ptr(out)) == 1
