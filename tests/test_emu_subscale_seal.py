"""CPU emulation of the sealed mod-down tail (tests/emu/emu_subscale_seal.cpp compiles subscale_seal.hpp, the per-word step the
kernels of subscale_sealed.hip call): the step's word and flags are checked_sub_scale's for every combination of present and absent
operands, the digests of a row are the seal Python integers give whatever the chunking and the merge order, a flipped input word
moves the input digest while the residue identity stays true, and a flip at the store leaves both digests alone -- without a GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

from helpers.emu_build import build_emu
from oracle import cport as O

p64 = C.POINTER(C.c_uint64)
p32 = C.POINTER(C.c_uint32)
P = (1 << 61) - 1
SUM, RANGE = 1, 2
PW_OPERAND = 4
LOAD, STORE = 0, 1
GARBAGE = 0x5A5A5A5A5A5A5A5A
N = 1 << 10


@pytest.fixture(scope="module")
def emu():
    L = build_emu("libemu_subscale_seal.so", ["emu_subscale_seal.cpp"], ("modarith.hpp", "residue_check.hpp", "baseconv_check.hpp",
                                                                         "keyswitch_check.hpp", "seal_check.hpp", "subscale_seal.hpp"))
    L.emu_subscale_word.restype = None
    L.emu_subscale_word.argtypes = [C.c_uint64] * 3 + [C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, p64]
    L.emu_subscale_row.restype = C.c_int
    L.emu_subscale_row.argtypes = [p64, p64, p64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_int, p64, p32,
                                   p64, p32]
    L.emu_subscale_verdict.restype = C.c_uint
    L.emu_subscale_verdict.argtypes = [p64, C.c_int, p64]
    L.emu_subscale_point_exists.restype = C.c_int
    L.emu_subscale_point_exists.argtypes = [C.c_int] * 3
    return L


def seal_of(x):
    """S0 = sum x_j, S1 = sum (j + 1) x_j modulo 2^61 - 1 in Python integers."""
    return [sum(int(v) for v in x) % P, sum((j + 1) * int(v) for j, v in enumerate(x)) % P]


def reference(x, y, add, s, q):
    """((x - y) s + add) mod q in Python integers; an absent operand is zero."""
    zero = [0] * N
    x, y, add = (zero if v is None else v for v in (x, y, add))
    return np.array([((int(a) - int(b)) * s + int(d)) % q for a, b, d in zip(x, y, add)], dtype=np.uint64)


class Data:
    """a 50-bit and a 61-bit modulus, each with a row of x, y and addend words in [16, q - 16), the row's constant and the references"""

    def __init__(self):
        self.rows = []
        for bits in (50, 61):
            q = int(O.gen_primes(2 * N, bits, 1)[0])
            rng = np.random.default_rng(bits)
            x, y, add = (rng.integers(16, q - 16, N, dtype=np.uint64) for _ in range(3))
            s = int(rng.integers(2, q - 1))
            self.rows.append((q, s, x, y, add, reference(x, y, add, s, q), seal_of(x)))


@pytest.fixture(scope="module")
def data():
    return Data()


def ptr(v):
    return v.ctypes.data_as(p64) if v is not None else None


def run(emu, x, y, add, s, q, form=3, log_chunk=8, lanes=64, reverse=0, hit=(-1, 0, 0)):
    """(out, residue flags, digests [[S0, S1] of x (IN), [S0, S1] of out (OUT)], range)"""
    out = np.zeros(N, dtype=np.uint64)
    fl, rng_ = C.c_uint32(0), C.c_uint32(0)
    dig = np.zeros(4, dtype=np.uint64)
    keep = [None if v is None else np.ascontiguousarray(v, dtype=np.uint64) for v in (x, y, add)]
    rc = emu.emu_subscale_row(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), N, s, q, form, log_chunk, lanes, reverse, hit[0], hit[1], hit[2], ptr(out), C.byref(fl),
                              ptr(dig), C.byref(rng_))
    assert rc == 0
    n = bin(form).count("1")
    return out, fl.value, [[int(v) for v in dig[2 * i:2 * i + 2]] for i in range(n)], rng_.value


def test_the_step_returns_checked_sub_scales_word_and_flags_for_every_operand_combination(emu, data):
    out = (C.c_uint64 * 4)()
    for q, s, x, y, add, _, _ in data.rows:
        words = [(int(x[0]), int(y[0]), int(add[0])), (int(y[1]), int(x[1]), int(add[1])), (0, q - 1, q - 1), (q - 1, 0, q - 1), (GARBAGE, int(y[2]), int(add[2])),
                 (int(x[3]), GARBAGE, 1), (int(x[4]), int(y[4]), GARBAGE)]
        for has, (a, b, d) in itertools.product(range(8), words):
            emu.emu_subscale_word(a, b, d, has, s, q, 7, out)
            assert (out[0], out[1]) == (out[2], out[3]), (q, has, a, b, d)
            present = [v for bit, v in zip((1, 2, 4), (a, b, d)) if has & bit]
            if all(v < q for v in present):
                want = (((a if has & 1 else 0) - (b if has & 2 else 0)) * s + (d if has & 4 else 0)) % q
                assert out[0] == want and out[1] == 0, (q, has, a, b, d)
            else:
                assert out[1] == PW_OPERAND, (q, has, a, b, d)      # flagged, not fixed


def test_a_rows_digests_are_the_seals_python_integers_give(emu, data):
    for q, s, x, y, add, want, seal_x in data.rows:
        out, fl, dig, rng_ = run(emu, x, y, add, s, q)
        assert (out == want).all() and fl == 0 and rng_ == 0
        assert dig == [seal_x, seal_of(want)]
        # the rescale's shape (no addend), the OUT form alone, the IN form alone
        want2 = reference(x, y, None, s, q)
        out, fl, dig, _ = run(emu, x, y, None, s, q)
        assert (out == want2).all() and fl == 0 and dig == [seal_x, seal_of(want2)]
        out, fl, dig, _ = run(emu, x, y, add, s, q, form=2)
        assert (out == want).all() and dig == [seal_of(want)]
        out, fl, dig, _ = run(emu, x, y, add, s, q, form=1)
        assert (out == want).all() and dig == [seal_x]
        stored = np.array(seal_x, dtype=np.uint64)
        d = np.array(dig[0], dtype=np.uint64)
        assert emu.emu_subscale_verdict(ptr(d), 0, ptr(stored)) == 0
        assert emu.emu_subscale_verdict(ptr(d), 0, None) == 0 and emu.emu_subscale_verdict(ptr(d), 1, None) == RANGE
        stored[0] += np.uint64(P)      # the same residue, not canonical: held word for word
        assert emu.emu_subscale_verdict(ptr(d), 0, ptr(stored)) == SUM


def test_the_results_do_not_depend_on_the_chunking_or_the_merge_order(emu, data):
    for q, s, x, y, add, want, seal_x in data.rows:
        base = run(emu, x, y, add, s, q, log_chunk=10, lanes=256)
        assert base[2] == [seal_x, seal_of(want)]
        for log_chunk, lanes, reverse in ((1, 1, 0), (3, 2, 1), (5, 64, 0), (8, 256, 1), (9, 128, 1), (10, 16, 0)):
            got = run(emu, x, y, add, s, q, log_chunk=log_chunk, lanes=lanes, reverse=reverse)
            assert (got[0] == base[0]).all() and got[1:] == base[1:], (log_chunk, lanes, reverse)


@pytest.mark.parametrize("j", [0, 255, 256, N - 1])
def test_a_flipped_input_word_moves_the_input_digest_and_leaves_the_residue_identity_true(emu, data, j):
    for q, s, x, y, add, want, seal_x in data.rows:
        for bit in (3, 20):      # x + 2^20 < q for x < q - 16 but one time in 2^30
            out, fl, dig, rng_ = run(emu, x, y, add, s, q, hit=(LOAD, j, bit))
            xf = x.copy()
            xf[j] ^= np.uint64(1 << bit)
            assert fl == 0 and rng_ == 0                      # a consistent operand of the identity: the gap the digest closes
            assert dig[0] == seal_of(xf) and dig[0][0] != seal_x[0] and dig[0][1] != seal_x[1]
            wf = reference(xf, y, add, s, q)
            assert (out == wf).all() and np.flatnonzero(out != want).tolist() == [j]
            assert dig[1] == seal_of(wf)                      # the output's seal is that of the words as stored
            stored, d = np.array(seal_x, dtype=np.uint64), np.array(dig[0], dtype=np.uint64)
            assert emu.emu_subscale_verdict(ptr(d), 0, ptr(stored)) == SUM
            # the same word changed in memory gives the same digests: the hook is a load of a changed word
            assert run(emu, xf, y, add, s, q)[2] == dig
        # a word >= q on the load: the window, PW_OPERAND in the residue flags
        out, fl, dig, rng_ = run(emu, x, y, add, s, q, hit=(LOAD, j, 63))
        assert rng_ == 1 and fl == PW_OPERAND


@pytest.mark.parametrize("j", [0, 255, 256, N - 1])
def test_a_flip_at_the_store_leaves_both_digests_alone(emu, data, j):
    for q, s, x, y, add, want, seal_x in data.rows:
        out, fl, dig, rng_ = run(emu, x, y, add, s, q, hit=(STORE, j, 3))
        assert fl == 0 and rng_ == 0 and dig == [seal_x, seal_of(want)]
        assert np.flatnonzero(out != want).tolist() == [j] and int(out[j]) == int(want[j]) ^ 8
        assert seal_of(out) != dig[1]                         # what the next verification sees
        out, fl, dig, _ = run(emu, x, y, add, s, q, form=2, hit=(STORE, j, 3))
        assert dig == [seal_of(want)] and int(out[j]) == int(want[j]) ^ 8


def test_a_point_needs_its_form(emu):
    assert emu.emu_subscale_point_exists(LOAD, 1, 1) and emu.emu_subscale_point_exists(STORE, 1, 1) and emu.emu_subscale_point_exists(STORE, 0, 1)
    assert not emu.emu_subscale_point_exists(LOAD, 0, 1) and not emu.emu_subscale_point_exists(STORE, 1, 0) and not emu.emu_subscale_point_exists(2, 1, 1)
