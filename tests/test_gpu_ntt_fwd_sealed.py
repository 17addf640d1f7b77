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
from helpers.sealed_ntt_runs import (GARBAGE, INVALID, POISON, RANGE, SUM, UNSUPPORTED, Case, check_raised, rows_of, run_between, run_clean, run_flips,
                                     run_inverse_without_output_seal)

pytestmark = pytest.mark.gpu

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


@pytest.fixture(scope="module")
def cases(F, eng):
    return case_cache(lambda logn: Case(F, eng, logn, SHAPES[logn]))


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
    run_inverse_without_output_seal(cases(logn), eng)


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
