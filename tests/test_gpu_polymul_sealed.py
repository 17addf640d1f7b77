"""The negacyclic product that verifies its factors' seals on the loads that transform them and writes its result's seal from the
words it stores (Abft.polymul_sealed), on the GPU: the words are the unchecked product's, a bit that rots in a factor at rest raises
exactly its row in exactly its factor's block and poisons exactly that row's output seal -- while the checked product's own block
stays clean over a wrong product: the gap, shown -- a fault on the product's own load is seen here and by nothing else, the checked
product's hooks poison through block 2, and the seal travels on into the sealed transforms.  Every comparison is ==.

Shapes, the smallest at which each code path exists: 2^5 (rows shorter than a wave), 2^10, 2^12 (the largest single launch), 2^13
(the smallest two-launch size; two polynomials from limb 1 on, a 61-bit prime among 50-bit ones: both arithmetic paths, a run
boundary and the slot addressing of flags, seals and partials), 2^14.  Operands are drawn from [16, q - 16).

And every size the product accepts, 2^5 .. 2^20 (polymul_fused_supported, ntt_kernels.hip: 5 <= logn <= NTT_MAX_LOGN = 20, which is
also the largest table set fhe_ntt_tables_create builds), in one shape -- the table set [50, 50, 61] from limb 1 on, two limbs, two
polynomials: four rows, both arithmetic paths, a run boundary -- through the clean, the rot-in-a-factor, the own-load, the flip-in-c
and the custody tests (ids "all-<logn>"); the own-load test there also hooks, for either factor, the words 2^k - 1 and 2^k for
every k and N - 1: a word on both sides of the first edge of any tile size."""
import numpy as np
import pytest

from helpers.sealed_case import case_cache, flip
from helpers.sealed_ntt_runs import pow2_words

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
SUM, RANGE = 1, 2
POISON = (1 << 64) - 1
GARBAGE = 0x5A5A5A5A5A5A5A5A
# logn: (limb bits of the table set, n_poly, start_idx)
SHAPES = {5: ([50, 50], 1, 0), 10: ([50, 50], 1, 0), 12: ([50, 50], 1, 0), 13: ([50, 61, 50, 50], 2, 1), 14: ([50, 50, 50], 1, 0)}
SIZES = list(SHAPES)
TWO_LAUNCH = [13, 14]
# every size the product accepts, in one four-row shape; a case key is then ("all", logn)
MAX_LOGN = 20
FOUR_ROWS = ([50, 50, 61], 2, 1)
EVERY_SIZE = SIZES + [pytest.param(("all", logn), id=f"all-{logn}") for logn in range(5, MAX_LOGN + 1)]


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


class Case:
    """a table set, its detector, two seeded factors [n_poly][limbs][N] on the host and on the device, their seals, and the
    references computed once: the unchecked product, the unchecked square of a, and their seals"""

    def __init__(self, F, eng, key):
        logn = key[1] if isinstance(key, tuple) else key
        bits, self.n_poly, self.start = FOUR_ROWS if isinstance(key, tuple) else SHAPES[key]
        self.logn, self.N = logn, 1 << logn
        self.qs = F.create_moduli(self.N, bits)
        self.limbs = len(bits) - self.start
        self.rows = self.n_poly * self.limbs
        self.kw = dict(limbs=self.limbs, start=self.start, n_poly=self.n_poly)
        self.t = eng.tables(logn, self.qs)
        self.ab = F.Abft(eng, self.t)
        rng = np.random.default_rng(2400 + logn)
        self.q_of = [self.qs[self.start + r % self.limbs] for r in range(self.rows)]
        self.a = np.stack([rng.integers(16, q - 16, self.N, dtype=np.uint64) for q in self.q_of])
        self.b = np.stack([rng.integers(16, q - 16, self.N, dtype=np.uint64) for q in self.q_of])
        self.da, self.db = eng.upload(self.a), eng.upload(self.b)
        self.seal_a, self.seal_b = self.t.seal(self.da, **self.kw), self.t.seal(self.db, **self.kw)
        self.c = self.unchecked(eng, self.da, self.db)
        self.sq = self.unchecked(eng, self.da, None)

    def copy(self, eng, d):
        w = eng.alloc(self.rows * self.N)
        w.copy_from(d)
        return w

    def unchecked(self, eng, da, db):
        """host words of polymul over copies of the factors (db None: the square of da)"""
        a = self.copy(eng, da)
        b = a if db is None else self.copy(eng, db)
        c = eng.alloc(self.rows * self.N)
        self.t.polymul(c, a, b, **self.kw)
        return c.download().reshape(self.rows, self.N)

    def factors(self, eng):
        return self.copy(eng, self.da), self.copy(eng, self.db)

    def seals_of(self, d):
        return self.t.seal(d, **self.kw).download().reshape(self.rows, 2)

    def words(self):
        """(row, word): word 0, both sides of the middle of a row, the last word"""
        return [(0, 0), (self.rows - 1, self.N // 2 - 1), (self.rows // 2, self.N // 2), (self.rows - 1, self.N - 1)]


@pytest.fixture(scope="module")
def cases(F, eng):
    return case_cache(lambda logn: Case(F, eng, logn))


def rows_of(d, c):
    return d.download().reshape(c.rows, c.N)


def check_flags(c, fl, a=(), b=(), checked=()):
    """exactly those rows raised in block a, in block b, and exactly those (row, word) pairs in the checked block"""
    assert fl["a"].shape == (c.rows,) and fl["b"].shape == (c.rows,) and fl["checked"].shape == (c.rows, 3)
    assert np.flatnonzero(fl["a"]).tolist() == sorted(a), fl
    assert np.flatnonzero(fl["b"]).tolist() == sorted(b), fl
    assert [tuple(int(v) for v in rc) for rc in np.argwhere(fl["checked"])] == sorted(checked), fl


def check_seal(c, dc, seal_c, poisoned):
    """exactly the rows in `poisoned` carry the poisoned pair, every other row fhe_seal's words; a sweep raises them and no other"""
    s = seal_c.download().reshape(c.rows, 2)
    want = c.seals_of(dc)
    for r in range(c.rows):
        assert s[r].tolist() == ([POISON, POISON] if r in poisoned else want[r].tolist()), r
    assert np.flatnonzero(c.t.seal_verify(dc, seal_c, **c.kw)).tolist() == sorted(poisoned)


def run(c, eng, a=None, b=None, alias=None, seal_a="own", seal_b="own", seal_out=True):
    """(dc, seal_c, flags) of one sealed product over copies of the case's factors (or the arrays given)"""
    fa, fb = c.factors(eng)
    a = fa if a is None else a
    b = fb if b is None else b
    dc = a if alias == "a" else b if alias == "b" else eng.alloc(c.rows * c.N)
    sa = c.seal_a if isinstance(seal_a, str) else seal_a
    sb = c.seal_b if isinstance(seal_b, str) else seal_b
    seal_c, fl = c.ab.polymul_sealed(dc, a, b, sa, sb, seal_out=seal_out, **c.kw)
    return dc, seal_c, fl


# ---- 1 ----
@pytest.mark.parametrize("logn", EVERY_SIZE)
def test_clean_fresh_aliased_squared_and_without_an_output_seal(eng, cases, logn):
    c = cases(logn)
    for alias in (None, "a", "b"):
        dc, seal_c, fl = run(c, eng, alias=alias)
        check_flags(c, fl)
        assert (rows_of(dc, c) == c.c).all(), alias
        assert (seal_c.download().reshape(c.rows, 2) == c.seals_of(dc)).all(), alias
    # squaring: one factor, one seal (given twice or once), block 1 repeats block 0
    for sb in (c.seal_a, None):
        a = c.copy(eng, c.da)
        dc, seal_c, fl = run(c, eng, a=a, b=a, seal_b=sb)
        check_flags(c, fl)
        assert (fl["b"] == fl["a"]).all() and (rows_of(dc, c) == c.sq).all()
        assert (seal_c.download().reshape(c.rows, 2) == c.seals_of(dc)).all()
    # no output seal asked for: none comes back, words and flags are the same
    dc, none, fl = run(c, eng, seal_out=False)
    check_flags(c, fl)
    assert none is None and (rows_of(dc, c) == c.c).all()
    # a stored seal that is wrong raises its row in its factor's block
    bad = c.seal_b.download().copy().reshape(c.rows, 2)
    bad[c.rows - 1] = GARBAGE
    dc, seal_c, fl = run(c, eng, seal_b=eng.upload(bad))
    check_flags(c, fl, b=[c.rows - 1])
    check_seal(c, dc, seal_c, [c.rows - 1])
    eng.check()


# ---- 2 ----
@pytest.mark.parametrize("logn", EVERY_SIZE)
def test_a_bit_that_rots_in_a_factor_raises_its_row_in_its_block_and_poisons_that_rows_seal(eng, cases, logn):
    c = cases(logn)
    for op in (0, 1):
        for (row, j), bit in zip(c.words(), (0, 40, 3, 63)):
            a, b = c.factors(eng)
            flip(eng, (a, b)[op], row * c.N + j, bit)
            want = c.unchecked(eng, a, b)
            dc, seal_c, fl = run(c, eng, a=a, b=b)
            check_flags(c, fl, **{"ab"[op]: [row]})           # and block 2 all zero: the gap
            f = int(fl["ab"[op]][row])
            assert f & SUM and bool(f & RANGE) == (bit == 63), (op, row, j, bit, f)
            check_seal(c, dc, seal_c, [row])
            got = rows_of(dc, c)
            assert (got == want).all()                        # the product of the factors as they are
            assert not (got[row] == c.c[row]).all() and (np.delete(got, row, 0) == np.delete(c.c, row, 0)).all()
    # squaring a rotten factor: both blocks carry its row
    a = c.copy(eng, c.da)
    row, j = c.words()[2]
    flip(eng, a, row * c.N + j, 3)
    dc, seal_c, fl = run(c, eng, a=a, b=a, seal_b=None)
    check_flags(c, fl, a=[row], b=[row])
    check_seal(c, dc, seal_c, [row])
    eng.check()


# ---- 3 ----
@pytest.mark.parametrize("logn", EVERY_SIZE)
def test_a_fault_on_the_products_own_load_is_seen_by_the_sealed_product_only(eng, cases, logn):
    c = cases(logn)
    for op in (0, 1):
        for row, j in c.words()[1:]:
            eng.inject_fault_polymul_sealed(op, row, j, 3)
            # the checked product does not run the step: silent, correct, and the hook stays armed
            a, b = c.factors(eng)
            dc = eng.alloc(c.rows * c.N)
            assert not c.ab.polymul_checked(dc, a, b, **c.kw).any()
            assert (rows_of(dc, c) == c.c).all()
            a, b = c.factors(eng)
            dc, seal_c, fl = run(c, eng, a=a, b=b)
            check_flags(c, fl, **{"ab"[op]: [row]})
            assert int(fl["ab"[op]][row]) == SUM
            check_seal(c, dc, seal_c, [row])
            got = rows_of(dc, c)
            assert not (got[row] == c.c[row]).all() and (np.delete(got, row, 0) == np.delete(c.c, row, 0)).all()
            if c.logn < 13:     # the single launch only reads its factors: memory is clean (two-launch sizes transform them in place)
                assert (rows_of(a, c) == c.a).all() and (rows_of(b, c) == c.b).all()
            else:               # what the fault computes is the product of the flipped word
                fa, fb = c.factors(eng)
                flip(eng, (fa, fb)[op], row * c.N + j, 3)
                assert (got == c.unchecked(eng, fa, fb)).all()
            dc, seal_c, fl = run(c, eng)      # one shot
            check_flags(c, fl)
            assert (rows_of(dc, c) == c.c).all()
    if isinstance(logn, tuple):
        # both sides of every power of two, alternating between row 0 and the last row: the product is that of the one flipped word
        for op in (0, 1):
            for i, j in enumerate(pow2_words(c.logn)):
                row = (0, c.rows - 1)[i & 1]
                eng.inject_fault_polymul_sealed(op, row, j, 3)
                dc, seal_c, fl = run(c, eng)
                check_flags(c, fl, **{"ab"[op]: [row]})
                assert int(fl["ab"[op]][row]) == SUM, (op, row, j)
                fa, fb = c.factors(eng)
                flip(eng, (fa, fb)[op], row * c.N + j, 3)
                got = rows_of(dc, c)
                assert (got == c.unchecked(eng, fa, fb)).all(), (op, row, j)
                assert not (got[row] == c.c[row]).all(), (op, row, j)
        dc, seal_c, fl = run(c, eng)          # one shot
        check_flags(c, fl)
        assert (rows_of(dc, c) == c.c).all()
    eng.check()


# ---- 4 ----
@pytest.mark.parametrize("logn", SIZES)
def test_the_checked_products_hooks_raise_block_2_and_poison_that_row(eng, cases, logn):
    from fhe_reliability_gpu_amd._lib import check, lib
    c = cases(logn)
    row, j = c.rows - 1, c.N // 2 + 5
    for point in ([0, 1, 2, 3] if logn in TWO_LAUNCH else [2]):
        check(lib.fhe_ctx_inject_fault_polymul(eng._h, point, row * c.N + j, 30))
        dc, seal_c, fl = run(c, eng)
        check_flags(c, fl, checked=[(row, 2 if point >= 2 else point)])
        check_seal(c, dc, seal_c, [row])
        assert not (rows_of(dc, c)[row] == c.c[row]).all()
        dc, seal_c, fl = run(c, eng)      # one shot
        check_flags(c, fl)
    eng.check()


# ---- 5 ----
@pytest.mark.parametrize("logn", EVERY_SIZE)
def test_a_bit_flipped_in_c_after_the_call_fails_its_seal_on_that_row_only(eng, cases, logn):
    c = cases(logn)
    dc, seal_c, fl = run(c, eng)
    check_flags(c, fl)
    assert not c.t.seal_verify(dc, seal_c, **c.kw).any()
    for row, j in c.words()[1:3]:
        flip(eng, dc, row * c.N + j, 3)
        assert np.flatnonzero(c.t.seal_verify(dc, seal_c, **c.kw)).tolist() == [row]
        flip(eng, dc, row * c.N + j, 3)
    eng.check()


# ---- 6 ----
@pytest.mark.parametrize("logn", SIZES)
def test_an_unsealed_factor_with_a_word_above_q_raises_the_window_and_keeps_the_unchecked_words(eng, cases, logn):
    c = cases(logn)
    a, b = c.factors(eng)
    row, j = c.rows - 1, c.N // 2
    flip(eng, a, row * c.N + j, 63)
    want = c.unchecked(eng, a, b)
    dc, seal_c, fl = run(c, eng, a=a, b=b, seal_a=None)
    assert fl["a"].tolist() == [RANGE if r == row else 0 for r in range(c.rows)]
    check_flags(c, fl, a=[row])
    assert (rows_of(dc, c) == want).all()
    check_seal(c, dc, seal_c, [row])
    eng.check()


# ---- 7 ----
@pytest.mark.parametrize("logn", [10, 13])
def test_refusals_leave_the_flag_buffer_untouched_and_take_the_hooks(F, eng, cases, logn):
    from fhe_reliability_gpu_amd._lib import check, lib
    c = cases(logn)
    a, b = c.factors(eng)
    dc, seal_c = eng.alloc(c.rows * c.N), eng.alloc(c.rows * 2)

    def raw(ab=c.ab, pa=None, pb=None, sb=None):
        fl = eng.upload(np.full(3 * c.rows + 8, GARBAGE, dtype=np.uint64))
        rc = lib.fhe_polymul_sealed(eng._h, dc.ptr, a.ptr if pa is None else pa, b.ptr if pb is None else pb, c.t._h, ab._h, c.n_poly, c.limbs, c.start,
                                    c.seal_a.ptr, c.seal_b.ptr if sb is None else sb, seal_c.ptr, fl.ptr, None)
        return rc, bool((fl.download() == GARBAGE).all())

    def arm():
        eng.inject_fault_polymul_sealed(0, 0, 0, 3)
        check(lib.fhe_ctx_inject_fault_polymul(eng._h, 2, 0, 3))

    def hooks_are_gone():
        return not any(v.any() for v in run(c, eng)[2].values())

    arm()
    eng.set_option("ntt_mode", 1)
    try:
        rc, untouched = raw()
    finally:
        eng.set_option("ntt_mode", 0)
    assert rc == UNSUPPORTED and untouched and hooks_are_gone()
    # a detector made for other tables
    arm()
    rc, untouched = raw(ab=F.Abft(eng, eng.tables(c.logn, c.qs)))
    assert rc == INVALID and untouched and "another table set" in lib.fhe_last_error().decode()
    assert hooks_are_gone()
    # a misaligned factor
    arm()
    rc, untouched = raw(pa=a.ptr.value + 8)
    assert rc == INVALID and untouched and "aligned" in lib.fhe_last_error().decode()
    assert hooks_are_gone()
    # squaring with another seal for b
    arm()
    rc, untouched = raw(pb=a.ptr, sb=c.seal_b.ptr)
    assert rc == INVALID and untouched and "squaring" in lib.fhe_last_error().decode()
    assert hooks_are_gone()
    # a hook row or word outside the call
    for bad in ((0, c.rows, 0, 3), (1, 0, c.N, 3)):
        eng.inject_fault_polymul_sealed(*bad)
        rc, untouched = raw()
        assert rc == INVALID and untouched and "outside the call" in lib.fhe_last_error().decode()
        assert hooks_are_gone()
    # operand 1 when squaring
    eng.inject_fault_polymul_sealed(1, 0, 0, 3)
    rc, untouched = raw(pb=a.ptr, sb=c.seal_a.ptr)
    assert rc == INVALID and untouched and "squaring" in lib.fhe_last_error().decode()
    assert hooks_are_gone()
    eng.check()


# ---- 8 ----
@pytest.mark.parametrize("logn", EVERY_SIZE)
def test_custody_from_seal_to_product_to_the_sealed_transforms(eng, cases, logn):
    c = cases(logn)
    a, b = c.factors(eng)
    sa, sb = c.t.seal(a, **c.kw), c.t.seal(b, **c.kw)
    dc, seal_c, fl = run(c, eng, a=a, b=b, seal_a=sa, seal_b=sb)
    check_flags(c, fl)
    assert not c.t.seal_verify(dc, seal_c, **c.kw).any()
    # c with seal_c is an accepted input of both sealed transforms
    for call in (c.t.ntt_sealed, c.t.intt_sealed_out):
        _, _, f2 = call(dc, seal_c, c.ab, **c.kw)
        assert not f2.any()
    eng.check()


# ---- 9 ----
def test_one_size_above_the_largest_there_is_no_table_set_to_call_with(F, eng):
    """polymul_fused_supported holds up to NTT_MAX_LOGN, which is also the largest table set: one size above MAX_LOGN the refusal is
    fhe_ntt_tables_create's (FHE_ERR_INVALID), so no call of the sealed product exists that could answer FHE_ERR_UNSUPPORTED"""
    qs = F.create_moduli(1 << MAX_LOGN, [50])
    with pytest.raises(F.FheError, match="bad table arguments"):
        eng.tables(MAX_LOGN + 1, qs)
    eng.check()
