"""Inputs that dictate the key switch's internals (tests/helpers/ks_worst_case.py), without a GPU: the helper's own congruences in
exact integers, the magnitudes its families reach (derived from the families, asserted for every committed seed and shape), and
the families fed to the CPU emulation libraries, which compile the kernels' own element functions: words equal Python-integer
results and no range window fires at the largest legal sums."""
import ctypes as C

import numpy as np
import pytest

from oracle import cport as O
from helpers import ks_worst_case as KW
from helpers.emu_build import build_emu

p64 = C.POINTER(C.c_uint64)
p32 = C.POINTER(C.c_uint32)
U = np.uint64
N = 1 << 16
PRIMES = {bits: O.gen_primes(N, bits, 4) for bits in (50, 61)}
TERMS = [1, 2, 7, 8, 9, 16, 17, 25]
PATHS = [("f64", 50), ("u64", 50), ("u64", 61)]
SLOTS = 512


def _emu(name, headers, protos):
    lib = build_emu(f"lib{name}.so", [f"{name}.cpp"], headers)
    for fn, args in protos.items():
        getattr(lib, fn).restype = C.c_int
        getattr(lib, fn).argtypes = args
    return lib


@pytest.fixture(scope="module")
def emu_ks():
    return _emu("emu_keyswitch_check", ("modarith.hpp", "residue_check.hpp", "baseconv_check.hpp", "keyswitch_check.hpp"), {
        "emu_ks_dot_checked": [p64, p64, C.c_int, C.c_size_t, C.c_uint64, C.c_int, C.c_int, C.c_int, p64, p32],
        "emu_ks_dot_plain": [p64, p64, C.c_int, C.c_size_t, C.c_uint64, C.c_int, p64],
        "emu_ks_tail_checked": [p64, p64, p64, C.c_int, C.c_size_t, C.c_uint64, C.c_uint64, C.c_int, C.c_int, p64, p32],
        "emu_ks_tail_plain": [p64, p64, p64, C.c_int, C.c_size_t, C.c_uint64, C.c_uint64, p64]})


@pytest.fixture(scope="module")
def emu_bsgs():
    return _emu("emu_bsgs_check", ("modarith.hpp", "residue_check.hpp", "baseconv_check.hpp", "keyswitch_check.hpp", "bsgs_check.hpp"), {
        "emu_diag_mac_checked": [p64, p64, p64, C.c_int, C.c_size_t, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, p64, p64, p32, p32],
        "emu_diag_mac_plain": [p64, p64, p64, C.c_int, C.c_size_t, C.c_uint64, C.c_int, p64, p64]})


@pytest.fixture(scope="module")
def emu_pw():
    return _emu("emu_pointwise", ("modarith.hpp", "residue_check.hpp"), {
        "emu_dot_checked": [p64, p64, C.c_int, C.c_size_t, C.c_uint64, C.c_int, C.c_int, C.c_int, p64, p32]})


@pytest.fixture(scope="module")
def emu_rs():
    return _emu("emu_rescale_check", ("modarith.hpp", "residue_check.hpp", "rescale_check.hpp"), {
        "emu_rescale_reduce_checked": [p64, C.c_size_t, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, p64, p32],
        "emu_rescale_reduce_plain": [p64, C.c_size_t, C.c_uint64, p64]})


def _u(x):
    return np.ascontiguousarray(x, dtype=U)


def _p(a):
    return a.ctypes.data_as(p64)


def _f(a):
    return a.ctypes.data_as(p32)


def _x_rows(q, terms, seed):
    """[terms][SLOTS] words != 0: random, with the first 32 slots at q - 1 in every term (the rows held at q - 1)"""
    rng = np.random.default_rng([seed, terms, q % 9973])
    x = rng.integers(1, q, (terms, SLOTS), dtype=U)
    x[:, :32] = q - 1
    return x


def _keys(x, q, path):
    """{name: y [terms][SLOTS]} of every family and of the same-sign block"""
    fam = [KW.product_families(x[t], q, path) for t in range(x.shape[0])]
    fam = [f[0] if path == "f64" else f for f in fam]
    keys = {name: np.stack([f[name] for f in fam]) for name in KW.FAMILIES}
    keys["same-sign"] = KW.same_sign_block(x, q, path)[0]
    return keys


def _dot_want(x, y, q):
    return [sum(int(x[t, i]) * int(y[t, i]) for t in range(x.shape[0])) % q for i in range(x.shape[1])]


# ---------------------------------------------------------------- the helper's own congruences
@pytest.mark.parametrize("path,bits", PATHS)
def test_family_words_satisfy_their_congruence(path, bits):
    q = PRIMES[bits][0]
    x = _x_rows(q, 1, 1)[0]
    out = KW.product_families(x, q, path)
    ys, terms = out if path == "f64" else (out, None)
    assert sorted(ys) == sorted(KW.FAMILIES)
    for name, y in ys.items():
        t = KW.family_target(name, q)
        for i in range(x.size):
            assert 0 <= int(y[i]) < q
            if t is None:
                assert int(y[i]) == q - 1
            else:
                assert int(x[i]) * int(y[i]) % q == t, (name, i)
        if terms is not None:
            # the design aid's term is the product's residue moved by a whole multiple of q, inside the kernel's claim |term| < 0.875 q
            for i in range(x.size):
                assert (int(terms[name][i]) - int(x[i]) * int(y[i])) % q == 0 and 8 * abs(int(terms[name][i])) < 7 * q, (name, i)
    if terms is not None:
        # both signs occur next to q / 2, and the far side of the rounding boundary is reached: a term of magnitude above q / 2
        near = np.stack([terms[n] for n in KW.NEAR_HALF])
        assert (near > 0).any() and (near < 0).any() and int(np.abs(near).max()) == (q + 3) // 2


def _plan_moduli(n, bits):
    got = {b: iter(O.gen_primes(n, b, bits.count(b))) for b in set(bits)}
    return [next(got[b]) for b in bits]


# (logn, L, K, dnum, bits of the L + K limbs, seed)
PLANS = [(6, 4, 2, 2, [50] * 4 + [61] * 2, 1), (6, 4, 1, 4, [50] * 5, 2), (7, 6, 3, 2, [61] * 9, 3), (6, 5, 3, 2, [50, 61, 50, 61, 50, 61, 50, 61], 4),
         (10, 4, 2, 2, [50] * 6, 5), (10, 4, 1, 4, [50] * 5, 6)]


def _dictated_plan(logn, L, K, dnum, bits, seed):
    n, M = 1 << logn, L + K
    qs = _plan_moduli(n, bits)
    rps = np.stack([O.root_powers(q, logn) for q in qs])
    alpha = -(-L // dnum)
    coef = np.zeros((L, n), dtype=U)
    for d in range(dnum):
        lo, hi = d * alpha, min(L, (d + 1) * alpha)
        others = [qs[j] for j in range(M) if j < lo or j >= hi]
        if hi - lo == 1:
            coef[lo] = KW.edge_coefficients(qs[lo], others, n, seed)
        else:
            coef[lo:hi] = KW.digit_columns(qs[lo:hi], others, n, seed)[0]
    c = O.nwt_forward_batch(coef, qs[:L], rps[:L])
    return qs, rps, coef, c


@pytest.mark.parametrize("logn,L,K,dnum,bits,seed", PLANS)
def test_extended_digits_and_solved_key_reproduce_the_dictated_accumulator(logn, L, K, dnum, bits, seed):
    n, M = 1 << logn, L + K
    qs, rps, coef, c = _dictated_plan(logn, L, K, dnum, bits, seed)
    x = KW.extended_digits(c, qs, L, K, dnum, logn, rps)
    # the opening INTT returns the chosen coefficients, and a digit's own limbs are the input's
    assert (O.nwt_inverse_batch(c, qs[:L], rps[:L]) == coef).all()
    alpha = -(-L // dnum)
    for d in range(dnum):
        assert (x[d, d * alpha:min(L, (d + 1) * alpha)] == c[d * alpha:min(L, (d + 1) * alpha)]).all()
    rng = np.random.default_rng(seed)
    y = np.stack([np.stack([np.stack([rng.integers(0, q, n, dtype=U) for q in qs]) for _ in range(2)]) for _ in range(dnum)])
    target = np.stack([np.stack([rng.integers(0, q, n, dtype=U) for q in qs]) for _ in range(2)])
    target[0, :, 0], target[1, :, 1] = 0, np.array([q - 1 for q in qs], dtype=U)
    key, undictated = KW.solve_key_for_acc(x, y, target, qs)
    assert undictated == 0
    for h in range(2):
        acc = None
        for d in range(dnum):
            acc = O.modmul_batch(x[d], key[d, h], qs, acc=acc)
        assert (acc == target[h]).all()
    assert (key < np.array(qs, dtype=U)[None, None, :, None]).all()


def test_solved_key_skips_zero_digits_and_counts_what_it_cannot_dictate():
    logn, L, K, dnum, bits, seed = PLANS[0]
    n = 1 << logn
    qs, rps, coef, c = _dictated_plan(logn, L, K, dnum, bits, seed)
    x = KW.extended_digits(c, qs, L, K, dnum, logn, rps)
    x[0, 2, 5] = 0                      # the second digit has to be solved there
    x[:, 3, 9] = 0                      # nothing to solve with: two words (one per half) stay as they are
    rng = np.random.default_rng(9)
    y = np.stack([np.stack([np.stack([rng.integers(0, q, n, dtype=U) for q in qs]) for _ in range(2)]) for _ in range(dnum)])
    target = np.stack([np.stack([rng.integers(1, q, n, dtype=U) for q in qs]) for _ in range(2)])
    key, undictated = KW.solve_key_for_acc(x, y, target, qs)
    assert undictated == 2
    assert (key[0, :, 2, 5] == y[0, :, 2, 5]).all() and (key[:, :, 3, 9] == y[:, :, 3, 9]).all()
    for h in range(2):
        acc = None
        for d in range(dnum):
            acc = O.modmul_batch(x[d], key[d, h], qs, acc=acc)
        ok = acc == target[h]
        assert not ok[3, 9] and ok.sum() == ok.size - 1


@pytest.mark.parametrize("bits", [50, 61])
@pytest.mark.parametrize("with_add", [False, True])
def test_tail_targets_hit_every_edge_on_the_oracles_difference(bits, with_add):
    q, p = PRIMES[bits][0], PRIMES[61][1]
    pinv = pow(p % q, -1, q)
    n = 256
    cn = np.random.default_rng(bits).integers(0, q, n, dtype=U)
    cn[:10] = [0, 0, q - 1, q - 1, 1, 0, q - 1, 5, 0, q - 1]
    acc, add = KW.tail_targets(cn, q, add=with_add, pinv=pinv, seed=3)
    assert (acc < U(q)).all() and (add is None) == (not with_add)
    qj = U(q)
    diff = (acc + (qj - cn)) % qj                                  # keyswitch_ref's own expression
    assert (diff == KW.tail_diff(acc, cn, q)).all()
    got = [int(v) for v in diff]
    for edge in (0, q - 1, 1, (q - 1) // 2, (q - p % q) % q):
        assert got.count(edge) >= 16, edge
    assert any(int(a) == int(b) for a, b in zip(acc, cn)) and any((int(a) + 1) % q == int(b) for a, b in zip(acc, cn))
    assert any(int(a) < int(b) for a, b in zip(acc, cn)) and any(int(a) > int(b) for a, b in zip(acc, cn))
    if with_add:
        assert (add < qj).all()
        v = [int(d) * pinv % q for d in got]
        sums = [a + int(b) for a, b in zip(v, add)]
        for s in (q - 1, q, 2 * q - 2):
            assert sums.count(s) >= 3, s
        assert max(sums) == 2 * q - 2


# ---------------------------------------------------------------- reach (derived from the families, not measured on a kernel)
@pytest.mark.parametrize("terms", [t for t in TERMS if t >= 8])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_same_sign_blocks_reach_the_largest_sums(terms, seed):
    """FP64: eight terms of one sign, each at least (q - 1) / 2 - 1 in magnitude, put the running sum at or above 4 q - 12 > 3.9 q
    before the first fold (the family allows about 8 (q - 1) / 2, a term on the far side of the rounding boundary (q + 3) / 2); the
    kernel's windows (|s| < 8 q before a fold, < min(terms, 8) q at the end) hold.  U64: eight products (q - 1)^2 before a fold."""
    q = PRIMES[50][0]
    x = _x_rows(q, terms, seed)
    y, (before, last) = KW.same_sign_block(x, q, "f64")
    assert before >= 3.9 * q, before / q
    assert before >= 4 * q - 12 and before < 8 * q and last < min(terms, 8) * q
    if terms <= 9:                      # one fold block: some slot has all eight terms on the far side of the rounding boundary
        assert before == 4 * q + 12
    # every term of a block on its slot's side
    t = np.stack([KW.f64_terms(x[i], y[i], q) for i in range(terms)])
    assert (t[:, 0::2] > 0).all() and (t[:, 1::2] < 0).all()
    for bits in (50, 61):
        q = PRIMES[bits][0]
        x = np.full((terms, 4), q - 1, dtype=U)
        y, (before, last) = KW.same_sign_block(x, q, "u64")
        assert (y == U(q - 1)).all() and 0 <= before - 8 * (q - 1) ** 2 < q and before < 1 << 128          # + the last fold's remainder


# ---------------------------------------------------------------- the families through the kernels' element functions
@pytest.mark.parametrize("path,bits", PATHS)
@pytest.mark.parametrize("terms", TERMS)
def test_inner_product_elements_are_exact_and_silent_on_every_family(emu_ks, emu_bsgs, emu_pw, path, bits, terms):
    q = PRIMES[bits][0]
    pid = 0 if path == "f64" else 1
    x = _u(_x_rows(q, terms, 7))
    x2 = _u(_x_rows(q, terms, 8))
    for name, y in _keys(x, q, path).items():
        y = _u(y)
        want = _dot_want(x, y, q)
        w, f = np.zeros(SLOTS, dtype=U), np.ones(SLOTS, dtype=np.uint32)
        assert emu_ks.emu_ks_dot_checked(_p(x), _p(y), terms, SLOTS, q, pid, -1, 0, _p(w), _f(f)) == 0
        assert [int(v) for v in w] == want, name
        assert not f.any(), f"{name}: flags {sorted(set(f[f != 0].tolist()))} at slots {np.flatnonzero(f)[:8].tolist()}"
        w = np.zeros(SLOTS, dtype=U)
        assert emu_ks.emu_ks_dot_plain(_p(x), _p(y), terms, SLOTS, q, pid, _p(w)) == 0
        assert [int(v) for v in w] == want, name
        # the BSGS inner sum: the diagonal words are the free factor, the two parts share them
        w0, w1 = np.zeros(SLOTS, dtype=U), np.zeros(SLOTS, dtype=U)
        f0, f1 = np.ones(SLOTS, dtype=np.uint32), np.ones(SLOTS, dtype=np.uint32)
        assert emu_bsgs.emu_diag_mac_checked(_p(y), _p(x), _p(x2), terms, SLOTS, q, pid, 0, -1, 0, _p(w0), _p(w1), _f(f0), _f(f1)) == 0
        assert [int(v) for v in w0] == want and [int(v) for v in w1] == _dot_want(x2, y, q), name
        assert not f0.any() and not f1.any(), name
        p0, p1 = np.zeros(SLOTS, dtype=U), np.zeros(SLOTS, dtype=U)
        assert emu_bsgs.emu_diag_mac_plain(_p(y), _p(x), _p(x2), terms, SLOTS, q, pid, _p(p0), _p(p1)) == 0
        assert (p0 == w0).all() and (p1 == w1).all(), name
        if terms <= 2:                  # the tensor's one- and two-term sums
            w, f = np.zeros(SLOTS, dtype=U), np.ones(SLOTS, dtype=np.uint32)
            assert emu_pw.emu_dot_checked(_p(x), _p(y), terms, SLOTS, q, pid, -1, 0, _p(w), _f(f)) == 0
            assert [int(v) for v in w] == want and not f.any(), name


@pytest.mark.parametrize("bits", [50, 61])
@pytest.mark.parametrize("with_add", [False, True])
def test_tail_element_is_exact_and_silent_on_every_edge(emu_ks, bits, with_add):
    q, p = PRIMES[bits][0], PRIMES[61][1]
    pinv = pow(p % q, -1, q)
    n = 1024
    cn = np.random.default_rng(bits + 1).integers(0, q, n, dtype=U)
    cn[:10] = [0, 0, q - 1, q - 1, 1, 0, q - 1, 5, 0, q - 1]
    acc, add = KW.tail_targets(cn, q, add=with_add, pinv=pinv, seed=4)
    a = _u(add) if with_add else np.zeros(1, dtype=U)
    want = [((int(acc[i]) - int(cn[i])) * pinv + (int(add[i]) if with_add else 0)) % q for i in range(n)]
    w, f = np.zeros(n, dtype=U), np.ones(n, dtype=np.uint32)
    assert emu_ks.emu_ks_tail_checked(_p(_u(acc)), _p(_u(cn)), _p(a), int(with_add), n, q, pinv, -1, 0, _p(w), _f(f)) == 0
    assert [int(v) for v in w] == want
    assert not f.any(), np.flatnonzero(f)[:8].tolist()
    w = np.zeros(n, dtype=U)
    assert emu_ks.emu_ks_tail_plain(_p(_u(acc)), _p(_u(cn)), _p(a), int(with_add), n, q, pinv, _p(w)) == 0
    assert [int(v) for v in w] == want


@pytest.mark.parametrize("last,rest", [(50, [50, 50, 50]), (61, [61, 61, 61]), (50, [50, 61, 50, 61]), (61, [50, 61, 50])])
def test_rescale_residues_of_edge_coefficients(emu_rs, last, rest):
    """x = [c]_{q_last} at the edges of every remaining prime: p - 1, p, p + 1, the multiples of p next to q_last, q_last - 1 -- on
    same-width plans the only coefficients for which x mod p differs from x"""
    qs = _plan_moduli(N, rest + [last])
    ql, others = qs[-1], qs[:-1]
    x = _u(KW.edge_coefficients(ql, others, 2048, seed=5))
    for p in others:
        for e in (p - 1, p, p + 1):
            assert e >= ql or e in [int(v) for v in x[:64]]
    for qj in others:
        w, f = np.zeros(x.size, dtype=U), np.ones(x.size, dtype=np.uint32)
        assert emu_rs.emu_rescale_reduce_checked(_p(x), x.size, ql, qj, -1, 0, _p(w), _f(f)) == 0
        assert [int(v) for v in w] == [int(v) % qj for v in x]
        assert not f.any(), (qj, np.flatnonzero(f)[:8].tolist())
        w = np.zeros(x.size, dtype=U)
        assert emu_rs.emu_rescale_reduce_plain(_p(x), x.size, qj, _p(w)) == 0
        assert [int(v) for v in w] == [int(v) % qj for v in x]
