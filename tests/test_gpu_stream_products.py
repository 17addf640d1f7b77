"""Products that need the conditional subtraction behind the 128-bit Barrett step, through every streaming call that multiplies:
fhe_modmul / _acc and their checked forms, fhe_scalar_affine and its checked form, fhe_tensor_product and its checked form,
fhe_bsgs_hadamard with a modulus and crt_garner.  Random canonical operands never bring barrett128()'s quotient estimate one short
(tests/test_stream_cases.py says for which moduli which words can); the rows here are filled with the pairs of
helpers/stream_cases.py that do -- a b mod q = 1, 2, 3, as canonical words and as the largest 64-bit words of the same classes --
each row with the pairs of its own modulus, padded with random words.  The FP64 limbs of the tensor product get the same family and
its mirror image (a b mod q = q - 1, q - 2): the two ends at which ArithF64::canonical()'s sign fix decides the word.

Every comparison is == against Python integers, and against oracle.cport where it has the call.  Tables: limbs of 50, 61, 30, 61,
50 bits at N = 2 and N = 2^10, the whole set and the window from limb 1 on, one and three polynomials.  Rows alternate between
canonical and lifted words: the checked calls raise no flag on a canonical row and exactly PW_OPERAND on a lifted one."""
import ctypes as C

import numpy as np
import pytest

from helpers import stream_cases as S
from oracle import cport as O

pytestmark = pytest.mark.gpu

BITS = [50, 61, 30, 61, 50]
LOGNS = [1, 10]
SHAPES = [(1, 0, 5), (3, 0, 5), (1, 1, 4), (3, 1, 4)]      # n_poly, start_idx, limbs
OPERAND = 4
SENTINEL = 0x5E5E5E5E5E5E5E5E
GARBAGE = 0xA5A5A5A5DEADBEEF
TOP = 2**64 - 1
DESIGNED = 48                                                # designed pairs at the head of a row (as many as N holds)


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


@pytest.fixture(scope="module")
def L():
    from fhe_reliability_gpu_amd._lib import lib
    return lib


@pytest.fixture(scope="module")
def tables(F, eng):
    made = {}

    def get(logn):
        if logn not in made:
            made[logn] = eng.tables(logn, F.create_moduli(1 << logn, BITS))
            assert set(made[logn].paths) == {0, 1}
        return made[logn]
    return get


def _is_lifted(poly, l, start):
    """rows alternate: over the four shapes every table limb is canonical in one case and lifted in another"""
    return (poly + l + start) % 2 == 1


def _layout(qs, n_poly, start):
    """(modulus, lifted) of every row of a batch [n_poly][limbs]"""
    return [(int(q), _is_lifted(p, l, start)) for p in range(n_poly) for l, q in enumerate(qs)]


def _random_words(rng, q, n, lifted):
    return rng.integers(0, TOP, n, dtype=np.uint64, endpoint=True) if lifted else rng.integers(0, q, n, dtype=np.uint64)


def _operands(layout, N, seed):
    """a, b as [rows + 1][N]: the designed pairs of the row's modulus at its head, starting at another pair in every row, random words
    behind them (canonical in a canonical row, any 64-bit word in a lifted one), and a sentinel row behind the batch"""
    rng = np.random.default_rng(seed)
    a, b = (np.empty((len(layout) + 1, N), dtype=np.uint64) for _ in range(2))
    for row, (q, lifted) in enumerate(layout):
        a[row], b[row] = _random_words(rng, q, N, lifted), _random_words(rng, q, N, lifted)
        pairs = S.small_residue_pairs(q, DESIGNED, rng, lift=lifted)
        for i in range(min(N, len(pairs))):
            a[row, i], b[row, i] = pairs[(i + row) % len(pairs)]
    a[-1] = b[-1] = SENTINEL
    return a, b


def _old_words(layout, N, seed):
    """the words an accumulate finds in c: canonical with q - 1 in every third column (a designed product of 1, 2 or 3 on top wraps),
    and in a lifted row any 64-bit word in the columns between"""
    rng = np.random.default_rng(seed)
    o = np.empty((len(layout) + 1, N), dtype=np.uint64)
    for row, (q, lifted) in enumerate(layout):
        o[row] = rng.integers(0, q, N, dtype=np.uint64)
        o[row, 0::3] = q - 1
        if lifted:
            o[row, 1::3] = rng.integers(0, TOP, len(o[row, 1::3]), dtype=np.uint64, endpoint=True)
    o[-1] = SENTINEL
    return o


def _ints(x):
    return x.astype(object)


def _q_column(layout):
    return np.array([q for q, _ in layout], dtype=object).reshape(-1, 1)


def _want_modmul(layout, a, b, o):
    """(a b + o) mod q per row: Python integers, and the C oracle's words, which have to agree"""
    q = _q_column(layout)
    want = (_ints(a[:-1]) * _ints(b[:-1]) + (0 if o is None else _ints(o[:-1]))) % q
    want = want.astype(np.uint64)
    for row, (m, _) in enumerate(layout):
        orc = O.modmul(a[row], b[row], m) if o is None else O.modmul_acc(o[row], a[row], b[row], m)
        assert (orc == want[row]).all()
    return want


def _run(eng, call, c, a, b):
    """c, a, b: host arrays, or the name of the operand that c (or b) aliases -> the words of every buffer after the call"""
    bufs = {}
    bufs["a"] = eng.upload(a)
    bufs["b"] = bufs["a"] if isinstance(b, str) else eng.upload(b)
    bufs["c"] = bufs[c] if isinstance(c, str) else eng.upload(c)
    assert call(bufs["c"].ptr, bufs["a"].ptr, bufs["b"].ptr) == 0
    eng.sync()
    return {k: v.download().reshape(a.shape) for k, v in bufs.items()}


def _assert_words(got, want):
    assert (got[-1] == SENTINEL).all(), "the call wrote behind its batch"
    bad = np.argwhere(got[:-1] != want)
    assert not len(bad), (bad[:8].tolist(), [hex(int(got[tuple(i)])) for i in bad[:8]], [hex(int(want[tuple(i)])) for i in bad[:8]])


def _designed_columns_are_short(layout, a, b, N):
    """the rows really carry what they were designed to carry: every designed lifted product, and most canonical ones of a modulus
    that canonical words can bring there, leave the estimate one short"""
    for row, (q, lifted) in enumerate(layout):
        n = min(N, DESIGNED)
        short = [S.barrett_shortfall(int(a[row, i]) * int(b[row, i]), q) for i in range(n)]
        if lifted:
            assert all(s == 1 for s in short)
        elif q.bit_length() > 32 and n > 2:
            assert 2 * sum(short) >= n


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("n_poly,start,limbs", SHAPES)
@pytest.mark.parametrize("logn", LOGNS)
def test_modmul(F, eng, L, tables, logn, n_poly, start, limbs, acc):
    t, N = tables(logn), 1 << logn
    layout = _layout(t.moduli[start:start + limbs], n_poly, start)
    seed = logn * 100 + n_poly * 10 + start
    a, b = _operands(layout, N, seed)
    _designed_columns_are_short(layout, a, b, N)
    o = _old_words(layout, N, seed + 1)
    f = L.fhe_modmul_acc if acc else L.fhe_modmul
    call = lambda c, x, y: f(eng._h, c, x, y, t._h, n_poly, limbs, start, None)
    # c separate: the operands stay as they were
    out = _run(eng, call, o if acc else np.full_like(a, SENTINEL), a, b)
    _assert_words(out["c"], _want_modmul(layout, a, b, o if acc else None))
    assert (out["a"] == a).all() and (out["b"] == b).all()
    # c = a, c = b: an accumulate then finds the operand as the old word
    _assert_words(_run(eng, call, "a", a, b)["c"], _want_modmul(layout, a, b, a if acc else None))
    _assert_words(_run(eng, call, "b", a, b)["c"], _want_modmul(layout, a, b, b if acc else None))
    # a = b
    _assert_words(_run(eng, call, o if acc else np.full_like(a, SENTINEL), a, "a")["c"], _want_modmul(layout, a, a, o if acc else None))


def _flags_buf(eng, n):
    return eng.upload(np.full((n + 1) // 2, GARBAGE, dtype=np.uint64))


def _read_flags(buf, n):
    return buf.download().view(np.uint32)[:n].copy()


def _want_flags(layout):
    return np.array([OPERAND if lifted else 0 for _, lifted in layout], dtype=np.uint32)


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("n_poly,start,limbs", SHAPES)
@pytest.mark.parametrize("logn", LOGNS)
def test_modmul_checked(F, eng, L, tables, logn, n_poly, start, limbs, acc):
    t, N = tables(logn), 1 << logn
    layout = _layout(t.moduli[start:start + limbs], n_poly, start)
    seed = logn * 100 + n_poly * 10 + start
    a, b = _operands(layout, N, seed)
    o = _old_words(layout, N, seed + 1)
    f = L.fhe_modmul_acc_checked if acc else L.fhe_modmul_checked
    flags = []

    def call(c, x, y):
        flags.append(_flags_buf(eng, len(layout)))
        return f(eng._h, c, x, y, t._h, n_poly, limbs, start, flags[-1].ptr, None)
    want_flags = _want_flags(layout)
    for c_, b_, old, bb in ((o if acc else np.full_like(a, SENTINEL), b, o, b), ("a", b, a, b), ("b", b, b, b),
                            (o if acc else np.full_like(a, SENTINEL), "a", o, a)):
        out = _run(eng, call, c_, a, b_)
        _assert_words(out["c"], _want_modmul(layout, a, bb, old if acc else None))
        got = _read_flags(flags[-1], len(layout))
        assert (got == want_flags).all(), (got.tolist(), want_flags.tolist())


# ---- scalar affine ------------------------------------------------------------------------------------------------------------
def _scalar_rows(layout, limbs, N, seed):
    """a as [rows + 1][N], base[l]: the head of every row of limb l holds one constant a_l from [q/2, q) (its largest 64-bit
    representative in a lifted row), so that the scalar s a_l^-1 brings the products of the whole head to s"""
    rng = np.random.default_rng(seed)
    base = [int(rng.integers(q // 2, q)) for q, _ in layout[:limbs]]
    a = np.empty((len(layout) + 1, N), dtype=np.uint64)
    for row, (q, lifted) in enumerate(layout):
        a[row] = _random_words(rng, q, N, lifted)
        v = base[row % limbs]
        a[row, :max(1, N // 2)] = S.lift(v, q) if lifted else v
    a[-1] = SENTINEL
    return a, base


@pytest.mark.parametrize("checked", [False, True])
@pytest.mark.parametrize("n_poly,start,limbs", SHAPES)
@pytest.mark.parametrize("logn", LOGNS)
def test_scalar_affine(F, eng, L, tables, logn, n_poly, start, limbs, checked):
    t, N = tables(logn), 1 << logn
    qs = t.moduli[start:start + limbs]
    layout = _layout(qs, n_poly, start)
    a, base = _scalar_rows(layout, limbs, N, logn * 100 + n_poly * 10 + start + 7)
    q = _q_column(layout)
    ia = _ints(a[:-1])
    arr = lambda v: None if v is None else (C.c_uint64 * limbs)(*v)
    col = lambda v: np.array([int(s) for s in v] * n_poly, dtype=object).reshape(-1, 1)
    want_flags = _want_flags(layout)
    case = 0
    for s in (1, 2, 3):
        mul = [s * pow(v, -1, m) % m for v, m in zip(base, qs)]
        # the head's product is s and the estimate one short (the 30-bit limb cannot get there: the call reduces its scalar, and a
        # 64-bit word times a 30-bit one stays below 2^94)
        for row, (m, lifted) in enumerate(layout):
            x = int(a[row, 0]) * mul[row % limbs]
            assert x % m == s and (S.barrett_shortfall(x, m) == 1 or m.bit_length() < 32)
        # no addend; an addend that brings the head to q exactly (-> 0) and one that stops at q - 1
        for add in (None, [m - s for m in qs], [m - 1 - s for m in qs]):
            given = mul if checked or case % 2 == 0 else [S.lift(v, m) for v, m in zip(mul, qs)]     # the plain call reduces its scalars
            want = ((ia * col(mul) + (0 if add is None else col(add))) % q).astype(np.uint64)
            flags = _flags_buf(eng, len(layout))
            if checked:
                call = lambda c, x, _y: L.fhe_scalar_affine_checked(eng._h, c, x, arr(given), arr(add), t._h, n_poly, limbs, start, flags.ptr, None)
            else:
                call = lambda c, x, _y: L.fhe_scalar_affine(eng._h, c, x, arr(given), arr(add), t._h, n_poly, limbs, start, None)
            if case % 2:                                # in place, as every internal caller uses it
                _assert_words(_run(eng, call, "a", a, "a")["c"], want)
            else:
                out = _run(eng, call, np.full_like(a, SENTINEL), a, "a")
                _assert_words(out["c"], want)
                assert (out["a"] == a).all()
            if checked:
                got = _read_flags(flags, len(layout))
                assert (got == want_flags).all(), (got.tolist(), want_flags.tolist())
            case += 1


# ---- tensor product -----------------------------------------------------------------------------------------------------------
def _tensor_patterns(q):
    """(a0 b1 mod q, a1 b0 mod q, a1 = a0): both cross terms from the family; one at 1 and the other at q - 1 (the sum is 0 mod q);
    with a1 = a0 the plain products d0 = a0 b0 and d2 = a1 b1 land on the second and the first residue as well; the mirror image
    next to q for the sign fix of the FP64 path"""
    return [(1, 2, False), (1, q - 1, False), (3, 1, True), (q - 1, q - 2, True), (2, 3, False), (q - 1, 1, False), (q - 2, q - 1, False),
            (2, 2, True), (q - 1, q - 1, True), (3, q - 3, False)]


def _tensor_operands(layout, N, seed):
    """a0, a1, b0, b1 as [limbs][N]"""
    rng = np.random.default_rng(seed)
    ops = [np.empty((len(layout), N), dtype=np.uint64) for _ in range(4)]
    for row, (q, lifted) in enumerate(layout):
        for x in ops:
            x[row] = _random_words(rng, q, N, lifted)
        pats = _tensor_patterns(q)
        for i in range(min(N, 4 * len(pats))):
            s1, s2, same = pats[(i + row) % len(pats)]
            a0 = int(rng.integers(q // 2, q))
            a1 = a0 if same else int(rng.integers(q // 2, q))
            b1, b0 = s1 * pow(a0, -1, q) % q, s2 * pow(a1, -1, q) % q
            assert a0 * b1 % q == s1 and a1 * b0 % q == s2
            for x, v in zip(ops, (a0, a1, b0, b1)):
                x[row, i] = S.lift(v, q) if lifted else v
    return ops


@pytest.mark.parametrize("checked", [False, True])
@pytest.mark.parametrize("start,limbs", [(0, 5), (1, 4)])
@pytest.mark.parametrize("logn", LOGNS)
def test_tensor_product(F, eng, L, tables, logn, start, limbs, checked):
    t, N = tables(logn), 1 << logn
    assert set(t.paths) == {0, 1} and set(t.paths[start:start + limbs]) == {0, 1}        # the FP64 and the integer path, both present
    layout = _layout(t.moduli[start:start + limbs], 1, start)
    host = _tensor_operands(layout, N, logn * 10 + start)
    a0, a1, b0, b1 = (_ints(x) for x in host)
    q = _q_column(layout)
    want = [(a0 * b0 % q).astype(np.uint64), ((a0 * b1 + a1 * b0) % q).astype(np.uint64), (a1 * b1 % q).astype(np.uint64)]
    for row, (m, _) in enumerate(layout):                            # the C oracle, term by term
        assert (O.modmul(host[0][row], host[2][row], m) == want[0][row]).all()
        assert (O.modmul_acc(O.modmul(host[0][row], host[3][row], m), host[1][row], host[2][row], m) == want[1][row]).all()
        assert (O.modmul(host[1][row], host[3][row], m) == want[2][row]).all()
    ops = [eng.upload(h) for h in host]
    d = [eng.upload(np.full((limbs + 1, N), SENTINEL, dtype=np.uint64)) for _ in range(3)]
    if checked:
        flags = _flags_buf(eng, 3 * limbs)
        rc = L.fhe_tensor_product_checked(eng._h, d[0].ptr, d[1].ptr, d[2].ptr, ops[0].ptr, ops[1].ptr, ops[2].ptr, ops[3].ptr, t._h, limbs, start,
                                          flags.ptr, None)
    else:
        rc = L.fhe_tensor_product(eng._h, d[0].ptr, d[1].ptr, d[2].ptr, ops[0].ptr, ops[1].ptr, ops[2].ptr, ops[3].ptr, t._h, limbs, start, None)
    assert rc == 0
    eng.sync()
    for k in range(3):
        _assert_words(d[k].download().reshape(limbs + 1, N), want[k])
    if checked:
        got = _read_flags(flags, 3 * limbs).reshape(limbs, 3)
        assert (got == np.repeat(_want_flags(layout), 3).reshape(limbs, 3)).all(), got.tolist()
    for x, h in zip(ops, host):
        assert (x.download().reshape(h.shape) == h).all()


# ---- BSGS Hadamard with a modulus ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lifted", [False, True])
@pytest.mark.parametrize("k", [1, 2, 9])
def test_bsgs_hadamard_mod(F, eng, L, tables, k, lifted):
    """y_i = sum_j M[(j - i) mod k] (.) v_j mod q with every term from the family: v_j[e] = t_j a_e, M_b[e] = s_b a_e^-1, so that the
    term (b, j) is s_b t_j -- 1 .. 6 -- and the sum depends on i.  From two blocks on, t_0 = -1: the running sum then stands just below
    q when the first short product arrives, and a product left unreduced is not absorbed by the sum's own conditional subtraction
    (with k = 1 it always is: acc = 0 + r, less q)"""
    bs = 300                                                          # two workgroups for k = 1, the last one partial
    for q in tables(10).moduli[:3]:                                   # 50, 61 and 30 bits
        rng = np.random.default_rng(k * 2 + lifted)
        base = [int(x) for x in rng.integers(q // 2, q, bs)]
        M = np.array([[(1 + b % 3) * pow(x, -1, q) % q for x in base] for b in range(k)], dtype=object)
        tj = [q - 1 if j == 0 and k > 1 else 1 + j % 2 for j in range(k)]
        v = np.array([[tj[j] * x % q for x in base] for j in range(k)], dtype=object)
        assert all(int(M[b, e]) * int(v[j, e]) % q == (1 + b % 3) * tj[j] % q for b in range(k) for j in range(k) for e in (0, bs - 1))
        if lifted:
            M, v = M + (TOP - M) // q * q, v + (TOP - v) // q * q
        short = [S.barrett_shortfall(int(M[b, e]) * int(v[j, e]), q) for b in range(k) for j in range(k > 1, k) for e in range(0, bs, 7)]
        assert all(s == 1 for s in short) if lifted else q.bit_length() < 32 or 2 * sum(short) >= len(short)
        want = np.empty((k, bs), dtype=object)
        for i in range(k):
            want[i] = sum(M[(j - i) % k] * v[j] for j in range(k)) % q
        Mw, vw = M.astype(np.uint64), v.astype(np.uint64)
        assert (O.bsgs_hadamard_mod(Mw, vw, q).reshape(k, bs) == want.astype(np.uint64)).all()
        dM, dv = eng.upload(Mw), eng.upload(vw)
        y = eng.upload(np.full((k + 1, bs), SENTINEL, dtype=np.uint64))
        assert L.fhe_bsgs_hadamard(eng._h, y.ptr, dM.ptr, dv.ptr, k, bs, q, None) == 0
        eng.sync()
        _assert_words(y.download().reshape(k + 1, bs), want.astype(np.uint64))


# ---- Garner ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [[30, 50, 61], [30, 50, 30, 61], [30, 61, 50]])
def test_crt_garner_digits_of_1_2_3(F, eng, bits):
    """residues of x = c_0 + c_1 p_0 + c_2 p_0 p_1 (+ ...) with c_j in {1, 2, 3} for j >= 1: the digit product t * inv_pref mod p_j lands
    on c_j.  The primes create_moduli returns lie just below powers of two, so a prefix product that is not much longer than p_j is a
    small number modulo p_j and the product t * inv_pref stays too short to bring the estimate one short: a 30-bit prime leads, and
    the last limb, whose prefix is tens of bits longer than itself, is the one where every designed digit needs the subtraction"""
    N = 300
    mods = F.create_moduli(1 << 10, bits)
    m = len(mods)
    rng = np.random.default_rng(sum(bits))
    res = np.stack([rng.integers(0, p, N, dtype=np.uint64) for p in mods])
    designed = 200
    short = {j: [] for j in range(1, m)}
    for i in range(designed):
        c = [int(rng.integers(0, mods[0]))] + [1 + (i + j) % 3 for j in range(1, m)]
        x, pref = 0, 1
        for j in range(m):
            x += c[j] * pref
            if j:
                t, inv = c[j] * (pref % mods[j]) % mods[j], pow(pref % mods[j], -1, mods[j])
                assert t * inv % mods[j] == c[j]
                short[j].append(S.barrett_shortfall(t * inv, mods[j]))
            pref *= mods[j]
        assert x < 1 << 128                # (no product of the recurrence wraps: the digits are the designed ones)
        res[:, i] = [x % p for p in mods]
    assert all(s == 1 for s in short[m - 1]) and len(short[m - 1]) == designed
    want_lo, want_hi = S.garner_python(res, mods)
    o_lo, o_hi = O.crt_garner(res, mods)
    assert (o_lo == want_lo).all() and (o_hi == want_hi).all()
    lo, hi = F.crt_garner(res, mods, eng)
    assert (lo == want_lo).all() and (hi == want_hi).all()
    # and the designed columns reconstruct x itself
    for i in range(0, designed, 17):
        x = int(lo[i]) | int(hi[i]) << 64
        assert [x % p for p in mods] == [int(r) for r in res[:, i]]
