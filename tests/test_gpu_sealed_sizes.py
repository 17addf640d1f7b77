"""The sealed transforms (ntt_sealed, intt_sealed_out, intt_sealed) at EVERY transform size 2^5 .. 2^20 on the GPU.  Each size is a
kernel of its own -- the single-pass sizes have their own register steps, from 2^13 on the column plan and the row-tile geometry
change again at 2^15, 2^17, 2^18, 2^19 and 2^20 -- and the seal tap's word weight, the hook's tile-relative index and the count of
partials per row all depend on it.  Every comparison is ==.

One shape at every size: the table set [50, 50, 61] from limb 1 on, two limbs, two polynomials -- four rows, both arithmetic
paths, a run boundary between them, slot addressing that is not the identity.  Operands are drawn from [16, q - 16), so that a
flipped bit 3 stays below q.

Besides the runners of test_gpu_ntt_fwd_sealed.py, unchanged: the output seal against S0 = sum x_j, S1 = sum (j + 1) x_j modulo
2^61 - 1 in Python integers (every row below 2^17, row 0 and the last row from there on), and a hook sweep over the words 2^k - 1
and 2^k for every k and N - 1, which puts a word on both sides of the first edge of any tile size without knowing the geometry and
holds the output against the unchecked transform of that one flipped word."""
import numpy as np
import pytest

from helpers.sealed_case import case_cache
from helpers.sealed_ntt_runs import (GARBAGE, UNSUPPORTED, Case, run_between, run_clean, run_clean_python_seal, run_flips, run_hook_sweep,
                                     run_inverse_without_output_seal)

pytestmark = pytest.mark.gpu

SHAPE = ([50, 50, 61], 2, 1)
SIZES = list(range(5, 21))
TWO_LAUNCH = [logn for logn in SIZES if logn >= 13]
DIRECTIONS = [pytest.param(False, id="forward"), pytest.param(True, id="inverse")]


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


@pytest.fixture(scope="module")
def cases(F, eng):
    return case_cache(lambda logn: Case(F, eng, logn, SHAPE))


@pytest.mark.parametrize("inv", DIRECTIONS)
@pytest.mark.parametrize("logn", SIZES)
def test_clean_in_place_and_out_of_place(eng, cases, logn, inv):
    run_clean(cases(logn), eng, inv)


@pytest.mark.parametrize("inv", DIRECTIONS)
@pytest.mark.parametrize("logn", SIZES)
def test_clean_output_seal_is_the_python_integer_seal(eng, cases, logn, inv):
    run_clean_python_seal(cases(logn), eng, inv)


@pytest.mark.parametrize("logn", SIZES)
def test_the_sealed_inverse_without_an_output_seal(eng, cases, logn):
    run_inverse_without_output_seal(cases(logn), eng)


@pytest.mark.parametrize("inv", DIRECTIONS)
@pytest.mark.parametrize("logn", SIZES)
def test_flips_in_source_memory_raise_and_poison_exactly_their_rows(eng, cases, logn, inv):
    run_flips(cases(logn), eng, inv)
    eng.check()


@pytest.mark.parametrize("inv", DIRECTIONS)
@pytest.mark.parametrize("logn", TWO_LAUNCH)
def test_flip_between_the_launches_raises_the_abft_word_and_poisons_that_row(eng, cases, logn, inv):
    run_between(cases(logn), eng, inv)


@pytest.mark.parametrize("inv", DIRECTIONS)
@pytest.mark.parametrize("logn", SIZES)
def test_hook_on_both_sides_of_every_power_of_two(eng, cases, logn, inv):
    run_hook_sweep(cases(logn), eng, inv)


@pytest.mark.parametrize("logn", [1, 2, 3, 4])
def test_below_2_to_the_5_the_sealed_calls_are_refused_with_nothing_launched(F, eng, logn):
    """N < 2^5 has no checked transform: every sealed transform and the sealed product return FHE_ERR_UNSUPPORTED, the flag buffer
    keeps the garbage it started with and no operand is touched"""
    from fhe_reliability_gpu_amd._lib import lib
    bits, n_poly, start = SHAPE
    N, limbs = 1 << logn, len(bits) - start
    rows = n_poly * limbs
    qs = F.create_moduli(N, bits)
    t = eng.tables(logn, qs)
    ab = F.Abft(eng, t)
    rng = np.random.default_rng(3000 + logn)
    x = np.stack([rng.integers(0, qs[start + r % limbs], N, dtype=np.uint64) for r in range(rows)])
    src, other, dst = eng.upload(x), eng.upload(x), eng.alloc(rows * N)
    seal = t.seal(src, limbs=limbs, start=start, n_poly=n_poly)
    seal_dst = eng.alloc(rows * 2)
    head = (eng._h, dst.ptr, src.ptr)
    shape = (t._h, ab._h, n_poly, limbs, start)
    calls = {
        "forward": lambda fl: lib.fhe_ntt_forward_sealed(*head, *shape, seal.ptr, seal_dst.ptr, fl.ptr, None),
        "inverse": lambda fl: lib.fhe_ntt_inverse_sealed(*head, *shape, seal.ptr, fl.ptr, None),
        "inverse_out": lambda fl: lib.fhe_ntt_inverse_sealed_out(*head, *shape, seal.ptr, seal_dst.ptr, fl.ptr, None),
        "product": lambda fl: lib.fhe_polymul_sealed(*head, other.ptr, *shape, seal.ptr, seal.ptr, seal_dst.ptr, fl.ptr, None),
    }
    for name, call in calls.items():
        fl = eng.upload(np.full(3 * rows + 8, GARBAGE, dtype=np.uint64))
        assert call(fl) == UNSUPPORTED, name
        assert (fl.download() == GARBAGE).all(), name
        assert (src.download().reshape(rows, N) == x).all() and (other.download().reshape(rows, N) == x).all(), name
    eng.check()
