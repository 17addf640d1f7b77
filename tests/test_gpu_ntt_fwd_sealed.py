"""The forward transform that verifies its input's seal on its own load and writes its output's seal from the words it stores
(ntt_sealed), and the sealed inverse with an output seal (intt_sealed_out), on the GPU: the words are the unchecked transforms',
corruptions at rest raise exactly their rows and poison exactly those rows' output seals, a fault on the transform's own load is
seen here and by nothing else, and a seal travels across a change of domain and back.  Every comparison is ==.

Shapes, the smallest at which each code path exists: 2^5 (rows shorter than a wave), 2^10, 2^12 (the largest single pass), 2^13
(the smallest two-launch size; two polynomials from limb 1 on, a 61-bit prime among 50-bit ones: both arithmetic paths, a run
boundary and the slot addressing of flags, seals and partials), 2^14.  Operands are drawn from [16, q - 16)."""
import numpy as np
import pytest

from helpers.sealed_case import case_cache, flip

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
SUM, RANGE = 1, 2
POISON = (1 << 64) - 1
GARBAGE = 0x5A5A5A5A5A5A5A5A
# logn: (limb bits of the table set, n_poly, start_idx)
SHAPES = {5: ([50, 50], 1, 0), 10: ([50, 50], 1, 0), 12: ([50, 50], 1, 0), 13: ([50, 61, 50, 50], 2, 1), 14: ([50, 50, 50], 1, 0)}
SIZES = list(SHAPES)
TWO_LAUNCH = [13, 14]
INV_SIZES = [10, 13, 14]


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


class Case:
    """a table set, its detector, seeded rows [n_poly][limbs][N] in both domains on the host and on the device, their seals"""

    def __init__(self, F, eng, logn):
        bits, self.n_poly, self.start = SHAPES[logn]
        self.logn, self.N = logn, 1 << logn
        self.qs = F.create_moduli(self.N, bits)
        self.limbs = len(bits) - self.start
        self.rows = self.n_poly * self.limbs
        self.kw = dict(limbs=self.limbs, start=self.start, n_poly=self.n_poly)
        self.t = eng.tables(logn, self.qs)
        self.ab = F.Abft(eng, self.t)
        rng = np.random.default_rng(1000 + logn)
        self.q_of = [self.qs[self.start + r % self.limbs] for r in range(self.rows)]
        self.x = np.stack([rng.integers(16, q - 16, self.N, dtype=np.uint64) for q in self.q_of])
        self.d = eng.upload(self.x)
        self.seal = self.t.seal(self.d, **self.kw)
        # the references, computed once: the unchecked forward transform of x, its seal, and both as the inverse's input
        self.dX = self.unchecked(eng, self.d, False)
        self.X = self.dX.download().reshape(self.rows, self.N)
        self.seal_X = self.t.seal(self.dX, **self.kw)

    def unchecked(self, eng, src, inv):
        w = eng.alloc(self.rows * self.N)
        w.copy_from(src)
        (self.t.inverse if inv else self.t.forward)(w, **self.kw)
        return w

    def side(self, inv):
        """(call, source, its seal, host words of the source, host words of the result)"""
        if inv:
            return self.t.intt_sealed_out, self.dX, self.seal_X, self.X, self.x
        return self.t.ntt_sealed, self.d, self.seal, self.x, self.X

    def seals_of(self, dst):
        return self.t.seal(dst, **self.kw).download().reshape(self.rows, 2)

    def words(self):
        """(row, word): word 0, both sides of the middle of a row (a tile edge of the row passes from 2^13 on), the last word"""
        return [(0, 0), (self.rows - 1, self.N // 2 - 1), (self.rows // 2, self.N // 2), (self.rows - 1, self.N - 1)]


@pytest.fixture(scope="module")
def cases(F, eng):
    return case_cache(lambda logn: Case(F, eng, logn))


def rows_of(dst, c):
    return dst.download().reshape(c.rows, c.N)


def check_raised(c, eng, dst, seal_dst, fl, rows, block):
    """exactly `rows` raised in `block` and nothing in the other one; exactly their seals poisoned, every other row's seal fhe_seal's;
    a sweep of dst against seal_dst raises them and no other row"""
    rows = sorted(rows)
    assert np.flatnonzero(fl[block]).tolist() == rows and not fl[1 - block].any(), fl
    s = seal_dst.download().reshape(c.rows, 2)
    want = c.seals_of(dst)
    for r in range(c.rows):
        assert s[r].tolist() == ([POISON, POISON] if r in rows else want[r].tolist()), r
    assert np.flatnonzero(c.t.seal_verify(dst, seal_dst, **c.kw)).tolist() == rows


def flips_scenarios(c, host):
    """[(name, [(row, word, bit)], rows that must carry SEAL_RANGE)]: single bits 0, 40 and 63; the reference's pattern, 3 symbols x 4
    bits in one row and spread over two rows; one word moved by +2^b - 2^(b + 32)"""
    r0, r1 = c.rows - 1, c.rows // 2 if c.rows // 2 != c.rows - 1 else 0
    N = c.N
    out = [("bit0", [(r0, 0, 0)], []), ("bit40", [(r1, N // 2, 40)], None), ("bit63", [(r0, N - 1, 63)], [r0])]
    sym = [(5, [1, 9, 17, 33]), (N // 2 + 3, [0, 13, 22, 47]), (N - 2, [2, 3, 30, 44])]
    out.append(("3x4 one row", [(r1, j, b) for j, bs in sym for b in bs], None))
    out.append(("3x4 two rows", [((r0, r1, r0)[i], j, b) for i, (j, bs) in enumerate(sym) for b in bs], None))
    b = 7
    j = next(j for j in range(N // 3, N) if not (int(host[r1][j]) >> b) & 1 and (int(host[r1][j]) >> (b + 32)) & 1)
    out.append(("fold-blind", [(r1, j, b), (r1, j, b + 32)], []))
    return out


def run_flips(c, eng, inv):
    call, src0, seal, host, _ = c.side(inv)
    src = eng.alloc(c.rows * c.N)
    src.copy_from(src0)
    for name, flips, ranged in flips_scenarios(c, host):
        for r, j, b in flips:
            flip(eng, src, r * c.N + j, b)
        try:
            dst, seal_dst, fl = call(src, seal, c.ab, **c.kw)
            want = c.unchecked(eng, src, inv)
        finally:
            for r, j, b in flips:
                flip(eng, src, r * c.N + j, b)
        rows = {r for r, _, _ in flips}
        check_raised(c, eng, dst, seal_dst, fl, rows, 0)
        assert all(int(fl[0][r]) & SUM for r in rows), (name, fl)
        if ranged is not None:
            assert [r for r in range(c.rows) if int(fl[0][r]) & RANGE] == ranged, (name, fl)
        assert (rows_of(dst, c) == rows_of(want, c)).all(), name      # the transform of the source as it is
    assert (src.download().reshape(-1) == src0.download().reshape(-1)).all()


def run_clean(c, eng, inv):
    call, src, seal, host, ref = c.side(inv)
    dst, seal_dst, fl = call(src, seal, c.ab, **c.kw)
    assert fl.shape == (2, c.rows) and not fl.any()
    assert (rows_of(dst, c) == ref).all()
    assert (src.download().reshape(c.rows, c.N) == host).all()              # out of place: the source is only read
    assert (seal_dst.download().reshape(c.rows, 2) == c.seals_of(dst)).all()
    w = eng.alloc(c.rows * c.N)
    w.copy_from(src)
    same_buf, seal_w, fl = call(w, seal, c.ab, dst=w, **c.kw)
    assert same_buf is w and not fl.any() and (rows_of(w, c) == ref).all()
    assert (seal_w.download() == seal_dst.download()).all()
    # no output seal asked for: none comes back, words and flags are the same
    dst, none, fl = call(src, seal, c.ab, seal_out=False, **c.kw)
    assert none is None and not fl.any() and (rows_of(dst, c) == ref).all()
    # a stored seal that is wrong raises its row; without one nothing is compared
    bad = seal.download().copy().reshape(c.rows, 2)
    bad[c.rows - 1] = GARBAGE
    dst, seal_dst, fl = call(src, eng.upload(bad), c.ab, **c.kw)
    check_raised(c, eng, dst, seal_dst, fl, [c.rows - 1], 0)
    dst, seal_dst, fl = call(src, None, c.ab, **c.kw)
    assert not fl.any() and (seal_dst.download().reshape(c.rows, 2) == c.seals_of(dst)).all()
    eng.check()


def run_between(c, eng, inv):
    from fhe_reliability_gpu_amd._lib import check, lib
    call, src, seal, _, ref = c.side(inv)
    row, j = c.rows - 1, c.N // 2 + 5
    check(lib.fhe_ctx_inject_fault(eng._h, row * c.N + j, 30))
    dst, seal_dst, fl = call(src, seal, c.ab, **c.kw)
    check_raised(c, eng, dst, seal_dst, fl, [row], 1)
    assert not (rows_of(dst, c) == ref).all()
    dst, seal_dst, fl = call(src, seal, c.ab, **c.kw)      # one shot
    assert not fl.any() and (rows_of(dst, c) == ref).all()
    eng.check()


# ---- 1 ----
@pytest.mark.parametrize("logn", SIZES)
def test_clean_in_place_and_out_of_place(eng, cases, logn):
    run_clean(cases(logn), eng, False)


# ---- 2 ----
@pytest.mark.parametrize("logn", SIZES)
def test_flips_in_source_memory_raise_and_poison_exactly_their_rows(eng, cases, logn):
    run_flips(cases(logn), eng, False)
    eng.check()


# ---- 3 ----
@pytest.mark.parametrize("logn", SIZES)
def test_a_fault_on_the_transforms_own_load_is_seen_by_the_sealed_transform_only(eng, cases, logn):
    c = cases(logn)
    for row, j in c.words():
        eng.inject_fault_ntt_sealed(row, j, 3)
        # the composition: a verifying sweep, then the checked forward on a copy -- silent, and the hook stays armed
        assert not c.t.seal_verify(c.d, c.seal, **c.kw).any()
        w = eng.alloc(c.rows * c.N)
        w.copy_from(c.d)
        assert not c.ab.forward_checked(w, **c.kw).any()
        assert (rows_of(w, c) == c.X).all()
        dst, seal_dst, fl = c.t.ntt_sealed(c.d, c.seal, c.ab, **c.kw)
        check_raised(c, eng, dst, seal_dst, fl, [row], 0)
        assert int(fl[0][row]) == SUM, (row, j, fl)
        assert (c.d.download().reshape(c.rows, c.N) == c.x).all()          # memory is clean
        got = rows_of(dst, c)
        assert not (got[row] == c.X[row]).all() and (np.delete(got, row, 0) == np.delete(c.X, row, 0)).all()
        dst, seal_dst, fl = c.t.ntt_sealed(c.d, c.seal, c.ab, **c.kw)      # one shot
        assert not fl.any() and (rows_of(dst, c) == c.X).all()
    eng.check()


# ---- 4 ----
@pytest.mark.parametrize("logn", TWO_LAUNCH)
def test_flip_between_the_launches_raises_the_abft_word_and_poisons_that_row(eng, cases, logn):
    run_between(cases(logn), eng, False)


# ---- 5 ----
@pytest.mark.parametrize("logn", SIZES)
def test_a_bit_flipped_in_dst_after_the_call_fails_its_seal_on_that_row_only(eng, cases, logn):
    c = cases(logn)
    dst, seal_dst, fl = c.t.ntt_sealed(c.d, c.seal, c.ab, **c.kw)
    assert not fl.any() and not c.t.seal_verify(dst, seal_dst, **c.kw).any()
    for row, j in c.words()[1:3]:
        flip(eng, dst, row * c.N + j, 3)
        assert np.flatnonzero(c.t.seal_verify(dst, seal_dst, **c.kw)).tolist() == [row]
        flip(eng, dst, row * c.N + j, 3)
    eng.check()


# ---- 6 ----
@pytest.mark.parametrize("logn", SIZES)
def test_an_unsealed_source_with_a_word_above_q_raises_the_window_and_keeps_the_unchecked_words(eng, cases, logn):
    c = cases(logn)
    src = eng.alloc(c.rows * c.N)
    src.copy_from(c.d)
    row, j = c.rows - 1, c.N // 2
    flip(eng, src, row * c.N + j, 63)
    dst, seal_dst, fl = c.t.ntt_sealed(src, None, c.ab, **c.kw)
    assert fl[0].tolist() == [RANGE if r == row else 0 for r in range(c.rows)] and not fl[1].any()
    assert (rows_of(dst, c) == rows_of(c.unchecked(eng, src, False), c)).all()
    assert seal_dst.download().reshape(c.rows, 2)[row].tolist() == [POISON, POISON]
    eng.check()


# ---- 7 ----
@pytest.mark.parametrize("logn", SIZES)
def test_round_trip_with_custody(eng, cases, logn):
    c = cases(logn)
    X, seal_X, fl = c.t.ntt_sealed(c.d, c.seal, c.ab, **c.kw)
    assert not fl.any()
    back, seal_back, fl = c.t.intt_sealed_out(X, seal_X, c.ab, **c.kw)
    assert not fl.any()
    assert (rows_of(back, c) == c.x).all()
    assert (seal_back.download() == c.seal.download()).all()
    # one bit flipped in the NTT-domain rows between the two calls: the inverse raises that row and poisons its output seal
    row, j = c.rows // 2, c.N // 2 + 1
    flip(eng, X, row * c.N + j, 3)
    back, seal_back, fl = c.t.intt_sealed_out(X, seal_X, c.ab, **c.kw)
    check_raised(c, eng, back, seal_back, fl, [row], 0)
    eng.check()


# ---- 8 ----
@pytest.mark.parametrize("logn", [10, 13])
def test_refusals_leave_the_flag_buffer_untouched_and_take_the_hook(F, eng, cases, logn):
    from fhe_reliability_gpu_amd._lib import lib
    c = cases(logn)
    dst, seal_dst = eng.alloc(c.rows * c.N), eng.alloc(c.rows * 2)

    def raw(ab=c.ab):
        fl = eng.upload(np.full(c.rows + 8, GARBAGE, dtype=np.uint64))
        rc = lib.fhe_ntt_forward_sealed(eng._h, dst.ptr, c.d.ptr, c.t._h, ab._h, c.n_poly, c.limbs, c.start, c.seal.ptr, seal_dst.ptr, fl.ptr, None)
        return rc, bool((fl.download() == GARBAGE).all())

    def hook_is_gone():
        return not c.t.ntt_sealed(c.d, c.seal, c.ab, **c.kw)[2].any()

    for name, on, off in (("ntt_mode", 1, 0), ("ntt_resident", 1, 0), ("ntt_packed", 1, 0), ("ntt_only_pass", 0, -1)):
        eng.inject_fault_ntt_sealed(0, 0, 3)
        eng.set_option(name, on)
        try:
            rc, untouched = raw()
        finally:
            eng.set_option(name, off)
        assert rc == UNSUPPORTED and untouched, name
        assert hook_is_gone(), name
    # a detector made for other tables
    other_t = eng.tables(c.logn, c.qs)
    eng.inject_fault_ntt_sealed(0, 0, 3)
    rc, untouched = raw(F.Abft(eng, other_t))
    assert rc == INVALID and untouched and "another table set" in lib.fhe_last_error().decode()
    assert hook_is_gone()
    # a hook row or word outside the call
    for bad in ((c.rows, 0, 3), (0, c.N, 3)):
        eng.inject_fault_ntt_sealed(*bad)
        rc, untouched = raw()
        assert rc == INVALID and untouched and "outside the call" in lib.fhe_last_error().decode()
        assert hook_is_gone()
    eng.check()


# ---- 9 ----
@pytest.mark.parametrize("logn", [10, 13])
def test_the_sealed_inverse_without_an_output_seal_is_unaffected(eng, cases, logn):
    c = cases(logn)
    dst, fl = c.t.intt_sealed(c.dX, c.seal_X, c.ab, **c.kw)
    assert not fl.any() and (rows_of(dst, c) == c.x).all()
    row, j = c.rows - 1, c.N // 2
    eng.inject_fault_ntt_sealed(row, j, 3)
    hooked, fl = c.t.intt_sealed(c.dX, c.seal_X, c.ab, **c.kw)
    assert np.flatnonzero(fl[0]).tolist() == [row] and int(fl[0][row]) == SUM and not fl[1].any()
    # the same fault through the call with an output seal: the same words and flags
    eng.inject_fault_ntt_sealed(row, j, 3)
    out, seal_out, fl2 = c.t.intt_sealed_out(c.dX, c.seal_X, c.ab, **c.kw)
    assert (fl2 == fl).all() and (rows_of(out, c) == rows_of(hooked, c)).all()
    # and what the fault computes is the transform of the flipped word
    y = eng.alloc(c.rows * c.N)
    y.copy_from(c.dX)
    flip(eng, y, row * c.N + j, 3)
    assert (rows_of(hooked, c) == rows_of(c.unchecked(eng, y, True), c)).all()
    eng.check()


# ---- 10 ----
@pytest.mark.parametrize("logn", INV_SIZES)
def test_inverse_with_output_seal_clean(eng, cases, logn):
    run_clean(cases(logn), eng, True)


@pytest.mark.parametrize("logn", INV_SIZES)
def test_inverse_with_output_seal_flips_in_source_memory(eng, cases, logn):
    run_flips(cases(logn), eng, True)
    eng.check()


@pytest.mark.parametrize("logn", TWO_LAUNCH)
def test_inverse_with_output_seal_flip_between_the_launches(eng, cases, logn):
    run_between(cases(logn), eng, True)
