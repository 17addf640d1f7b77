"""CPU emulation of the sealed tensor product (tests/emu/emu_tensor_seal.cpp compiles tensor_seal.hpp, the per-word step and the
per-row decision the kernels of tensor_sealed.hip call): the words are the tensor product's on both arithmetic paths, the seven
digests equal Python-integer sums whatever the chunking, the lanes and the order of merging, and a fault on the load moves exactly
the digest of the operand it hits while the residue identity goes on holding -- without a GPU.

Every expected value is a Python integer computed here."""
import ctypes as C

import numpy as np
import pytest

from helpers.emu_build import build_emu
from helpers.stream_cases import barrett_shortfall, fp64_edge_pairs, small_residue_pairs
from oracle import cport as O

p64, p32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
P = (1 << 61) - 1
SUM, RANGE = 1, 2
F64, U64 = 0, 1
# (bits, path): the FP64-term form exists below 2^50 only
PATHS = [(50, F64), (50, U64), (61, U64)]
LOGNS = [1, 5, 13, 14]
PRIMES = {(bits, logn): O.gen_primes(1 << logn, bits, 1)[0] for bits in (50, 61) for logn in LOGNS}


@pytest.fixture(scope="module")
def emu():
    L = build_emu("libemu_tensor_seal.so", ["emu_tensor_seal.cpp"], ("modarith.hpp", "residue_check.hpp", "seal_check.hpp", "tensor_seal.hpp"))
    L.emu_tensor_sealed.restype = C.c_int
    L.emu_tensor_sealed.argtypes = [p64, p64, p64, p64, C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int, p64, C.c_int, C.c_uint32,
                                    C.c_int, p64, p64, p64, p32, p64, p32]
    return L


def sums(x):
    """[S0, S1] of a row, Python integers"""
    row = [int(v) for v in x]
    return [sum(row) % P, sum((j + 1) * v for j, v in enumerate(row)) % P]


def product(ops, q):
    """fhe_tensor_product's words for any 64-bit operands, Python integers"""
    a0, a1, b0, b1 = ([int(v) for v in x] for x in ops)
    return ([x * y % q for x, y in zip(a0, b0)], [(w * z + x * y) % q for w, x, y, z in zip(a0, a1, b0, b1)], [x * y % q for x, y in zip(a1, b1)])


def sealed(emu, ops, q, path, log_chunk=None, lanes=256, reverse=False, out=True, seal=None, hit=(-1, 0, -1)):
    """(words [3], residue flags [3], digests [7 or 4][2], operand flags [4]); seal defaults to the true sums of the operands"""
    ops = [np.ascontiguousarray(x, dtype=np.uint64) for x in ops]
    n = ops[0].size
    log_chunk = min(n.bit_length() - 1, 13) if log_chunk is None else log_chunk
    seal = np.array([sums(x) for x in ops] if seal is None else seal, dtype=np.uint64).reshape(8)
    d = [np.full(n, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64) for _ in range(3)]
    fl, sf = np.full(3, 0xA5A5A5A5, dtype=np.uint32), np.full(4, 0xA5A5A5A5, dtype=np.uint32)
    dig = np.full(14, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    u = lambda a: a.ctypes.data_as(p64)
    rc = emu.emu_tensor_sealed(u(ops[0]), u(ops[1]), u(ops[2]), u(ops[3]), n, q, path, log_chunk, lanes, int(reverse), int(out), u(seal), hit[0], hit[1],
                               hit[2], u(d[0]), u(d[1]), u(d[2]), fl.ctypes.data_as(p32), u(dig), sf.ctypes.data_as(p32))
    assert rc == 0
    k = 7 if out else 4
    return d, fl.tolist(), [[int(v) for v in dig[2 * i:2 * i + 2]] for i in range(k)], sf.tolist()


def random_ops(rng, q, n, lo=0, hi=None):
    return [rng.integers(lo, q if hi is None else hi, n, dtype=np.uint64) for _ in range(4)]


def designed(rng, q, n, path):
    """(name, operands): the rows the reduction has to get right"""
    full = lambda v: np.full(n, v, dtype=np.uint64)
    rows = [("random", random_ops(rng, q, n)), ("all q - 1", [full(q - 1)] * 4), ("all zero", [full(0)] * 4),
            ("q - 1 against 1", [full(q - 1), full(1), full(1), full(q - 1)])]
    # products next to a multiple of q: Barrett's estimate is one short there, and the FP64 form's sign fix decides the word
    pairs = small_residue_pairs(q, n, rng) if path == U64 else fp64_edge_pairs(q, n, rng)
    a, b = np.array([p[0] for p in pairs], dtype=np.uint64), np.array([p[1] for p in pairs], dtype=np.uint64)
    rows.append(("small residues", [a, a.copy(), b, b.copy()]))
    return rows


@pytest.mark.parametrize("bits,path", PATHS)
def test_words_are_the_tensor_products_on_both_paths(emu, bits, path):
    for logn in (5, 13):
        n, q = 1 << logn, PRIMES[bits, logn]
        rng = np.random.default_rng(bits + path + logn)
        reached = False
        for name, ops in designed(rng, q, n, path):
            assert all((x < np.uint64(q)).all() for x in ops)
            want = product(ops, q)
            if name == "all q - 1":
                assert want[0] == [1] * n and want[1] == [2] * n
            if name == "small residues" and path == U64:
                reached = any(barrett_shortfall(int(x) * int(y), q) for x, y in zip(ops[0], ops[2]))
            d, fl, dig, sf = sealed(emu, ops, q, path)
            assert [x.tolist() for x in d] == [list(w) for w in want], name
            assert fl == [0, 0, 0] and sf == [0, 0, 0, 0], name
            assert dig == [sums(x) for x in ops] + [sums(w) for w in want], name
        assert reached or path == F64, "the designed pairs never needed Barrett's conditional subtraction"


@pytest.mark.parametrize("logn", LOGNS)
def test_seven_digests_equal_python_sums(emu, logn):
    n = 1 << logn
    for bits, path in PATHS:
        q = PRIMES[bits, logn]
        ops = random_ops(np.random.default_rng(100 * logn + bits + path), q, n)
        want = product(ops, q)
        for out in (True, False):
            d, fl, dig, sf = sealed(emu, ops, q, path, out=out)
            assert dig == ([sums(x) for x in ops] + [sums(w) for w in want])[:7 if out else 4]
            assert [x.tolist() for x in d] == [list(w) for w in want] and fl == [0, 0, 0] and sf == [0, 0, 0, 0]


def test_digests_do_not_depend_on_chunks_lanes_or_merge_order(emu):
    n, q = 1 << 14, PRIMES[61, 14]
    ops = random_ops(np.random.default_rng(14), q, n)
    ref = sealed(emu, ops, q, U64)
    assert ref[2][:4] == [sums(x) for x in ops]
    for log_chunk, lanes, reverse in ((13, 256, True), (14, 256, False), (9, 256, True), (6, 64, False), (1, 1, True), (13, 1024, False), (4, 2, True)):
        got = sealed(emu, ops, q, U64, log_chunk=log_chunk, lanes=lanes, reverse=reverse)
        assert got[2] == ref[2] and got[3] == [0, 0, 0, 0], (log_chunk, lanes, reverse)
        assert all((x == y).all() for x, y in zip(got[0], ref[0]))
    # logn = 1: one lane, two words
    n, q = 2, PRIMES[50, 1]
    ops = random_ops(np.random.default_rng(1), q, n)
    assert sealed(emu, ops, q, F64, log_chunk=1, lanes=256)[2] == sealed(emu, ops, q, F64, log_chunk=1, lanes=1)[2]


@pytest.mark.parametrize("bits,path", PATHS)
def test_a_fault_on_the_load_moves_its_operands_digest_only(emu, bits, path):
    for logn, log_chunk in ((5, 5), (14, 13)):
        n, q = 1 << logn, PRIMES[bits, logn]
        ops = random_ops(np.random.default_rng(7 * bits + logn + path), q, n, lo=16, hi=q - 16)      # bit 3 never leaves the window
        clean = sealed(emu, ops, q, path, log_chunk=log_chunk)
        for o in range(4):
            for coeff in (0, n // 2 - 1, n // 2, n - 1):
                for bit in (3, bits - 2):
                    hitw = int(ops[o][coeff]) ^ (1 << bit)
                    d, fl, dig, sf = sealed(emu, ops, q, path, log_chunk=log_chunk, hit=(o, coeff, bit))
                    where = (o, coeff, bit)
                    assert sf == [(SUM | (RANGE if hitw >= q else 0)) if i == o else 0 for i in range(4)], where
                    assert fl == ([0, 0, 0] if hitw < q else [4 if part in ((0, 1), (1, 2), (0, 1), (1, 2))[o] else 0 for part in range(3)]), where
                    faulted = [x.copy() for x in ops]
                    faulted[o][coeff] = hitw
                    assert dig[o] == sums(faulted[o]) and all(a != b for a, b in zip(dig[o], clean[2][o])), where
                    assert all(dig[i] == clean[2][i] for i in range(4) if i != o), where
                    want = product(faulted, q)
                    assert [x.tolist() for x in d] == [list(w) for w in want], where
                    assert dig[4:] == [sums(w) for w in want], where
        # the hook is a function of the armed word alone: none armed, nothing raised
        assert clean[3] == [0, 0, 0, 0] and clean[1] == [0, 0, 0]


@pytest.mark.parametrize("bits,path", PATHS)
def test_at_rest_changes_raise_their_row(emu, bits, path):
    logn = 14
    n, q = 1 << logn, PRIMES[bits, logn]
    rng = np.random.default_rng(bits + path)
    ops = random_ops(rng, q, n, lo=16, hi=q - 16)
    seal = [sums(x) for x in ops]
    for o in range(4):
        # one word, both sides of the chunk edge and the row's ends: the sum bit on that operand only; the identity holds
        for j in (0, (1 << 13) - 1, 1 << 13, n - 1):
            now = [x.copy() for x in ops]
            now[o][j] ^= np.uint64(8)
            d, fl, dig, sf = sealed(emu, now, q, path, seal=seal)
            assert sf == [SUM if i == o else 0 for i in range(4)] and fl == [0, 0, 0], (o, j)
            assert [x.tolist() for x in d] == [list(w) for w in product(now, q)], (o, j)
        # x -> x + p: no sum moves, the window alone sees it (the word is not fixed: the product is that of the word as it is)
        now = [x.copy() for x in ops]
        j = 1234 + o
        assert int(now[o][j]) + P < 1 << 64
        now[o][j] += np.uint64(P)
        d, fl, dig, sf = sealed(emu, now, q, path, seal=seal)
        assert sf == [RANGE if i == o else 0 for i in range(4)], o
        assert dig[:4] == seal, o
        assert [x.tolist() for x in d] == [list(w) for w in product(now, q)], o
        # two words by +d and -d: S0 does not move, S1 does
        now = [x.copy() for x in ops]
        now[o][100] += np.uint64(5)
        now[o][100 + 255 * 20] -= np.uint64(5)
        assert sums(now[o])[0] == seal[o][0]
        assert sealed(emu, now, q, path, seal=seal)[3] == [SUM if i == o else 0 for i in range(4)], o
        # a changed seal word, and a stored sum that is not canonical
        for w in (0, 1):
            bad = [list(s) for s in seal]
            bad[o][w] ^= 1 << 17
            assert sealed(emu, ops, q, path, seal=bad)[3] == [SUM if i == o else 0 for i in range(4)], (o, w)
        if seal[o][0] + P < 1 << 64:
            bad = [list(s) for s in seal]
            bad[o][0] += P
            assert sealed(emu, ops, q, path, seal=bad)[3] == [SUM if i == o else 0 for i in range(4)], o
