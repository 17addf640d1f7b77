"""The exact base conversion (fhe_baseconv_exact) at the digits that push its FP64 split sums to their exactness bounds, at every
fixed input size m = 1 .. 16 on both arithmetic paths, on the cold out-of-range branch, on a grid long enough for a second trip through
the coefficient loop, and -- in a child process with FHE_BC_VARIANT=0 -- through the runtime-m kernels that are the documented
fallback for m <= 16.  Every comparison is ==, against Python-integer arithmetic (tests/helpers/bc_worst_case.py) on the worst
columns and against the C oracle on all columns.

Per-workgroup output counts.  The fixed-size kernels accumulate OU outputs side by side (OU = 4 for m <= 11, 2 above) and a
workgroup whose output count is no multiple of OU recomputes its last output in the tail.  With N = 300 (two workgroups along N)
the launcher cuts the k outputs into slices while that gives fewer than 1024 workgroups and a slice keeps at least (m + 1) / 2
outputs; the counts per workgroup ("a,b": the slices but the last, the last) are

      m   OU   k = 1   k = 3   k = 6   k = 8   k = 13
    1, 2   4     1      1,2      2       1      1,2
    3, 4   4     1       3       3       2      1,4
    5, 6   4     1       3       3       4      1,4
    7, 8   4     1       3       6       4      6,7
    9-11   4     1       3       6       8      6,7
     12    2     1       3       6       8      6,7
    13-16  2     1       3       6       8      13

so that for OU = 4 the count is 0 mod 4 at (m = 5, k = 8) and (m = 9, k = 8), 1 at k = 1, 2 at (m = 1, k = 6), (m = 3, k = 8) and
(m = 7, k = 6), 3 at (m = 3, k = 3) and (m = 7, k = 13); for OU = 2 it is even at k = 6 and 8 and odd at k = 1, 3 and 13 (and both
in one launch at m = 12, k = 13).  Counts below OU: 1, 2 and 3 for OU = 4, 1 for OU = 2.  Nothing here asserts the launcher's
rule: the table only says which case reaches which tail.

Magnitudes the worst columns reach on the all-50-bit plans of this file (exact integers over the first eight terms, the span the
kernels accumulate before their first fold; bound 2^53): test_worst_columns_are_in_the_regime."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import bc_edge_cases as E
from helpers import bc_worst_case as W
from oracle import cport as O

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "bc_variant0_child.py")


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


def _bad_columns(got, want, names):
    """names (or indices) of the columns where two [k][columns] arrays differ"""
    return [names[i] if i < len(names) else int(i) for i in np.nonzero((got != want).any(axis=0))[0]]


def _check_case(F, eng, mi, mo, x, names, want_worst, what):
    N, k, n_w = x.shape[1], len(mo), len(names)
    bc = F.BaseConv(eng, mi, mo)
    d_in, d_out = eng.upload(x), eng.alloc(k * N)
    bc.exact(d_out, d_in, N)
    got = d_out.download().reshape(k, N).copy()
    assert not _bad_columns(got[:, :n_w], want_worst, names), (what, "against Python integers", _bad_columns(got[:, :n_w], want_worst, names))
    want = O.baseconv_exact(x, mi, mo)
    assert (want[:, :n_w] == want_worst).all(), what
    assert not _bad_columns(got, want, names), (what, "against the oracle", _bad_columns(got, want, names))
    # the checked call runs the Shoup form on every plan: FP64 against integer arithmetic on the same words
    d_chk = eng.alloc(k * N)
    flags = bc.exact_checked(d_chk, d_in, N)
    assert not flags.any(), (what, flags)
    chk = d_chk.download().reshape(k, N)
    assert not _bad_columns(chk, got, names), (what, "checked against plain", _bad_columns(chk, got, names))


@pytest.mark.parametrize("big", [False, True], ids=["f64", "u64"])
@pytest.mark.parametrize("m", range(1, 17))
def test_every_fixed_size_on_worst_and_random_columns(F, eng, m, big):
    for k in E.KS:
        mi, mo, x, names, want_worst = E.small_case(F, m, k, big)
        assert all(p < 1 << 50 for p in mi + mo) != big
        _check_case(F, eng, mi, mo, x, names, want_worst, f"m = {m}, k = {k}")


def test_worst_columns_are_in_the_regime(F):
    """The inputs above, not the kernel: over the first eight limbs (what the kernels sum before their first fold) the worst columns
    of the 50-bit plans put S2 past 2^51 and |S1| past 2^50, where uniformly random digits average 2^50 and 2^48.5.  Largest
    values over m = 8 .. 16 and k in KS, as this test prints them: S2 = 5746412201443328 = 2^52.352 and |S1| = 4355639077765120 =
    2^51.952, of the bound 2^53 (and S0, sixteen terms never folded, 2639123252772864 = 2^51.229 of its bound 2^52)."""
    s2 = s1 = 0
    for m in range(8, 17):
        for k in E.KS:
            mi, mo = E.moduli(F, m, k, False)
            cols = dict(W.worst_columns(mi, mo))
            for o, q in enumerate(mo):
                s2 = max(s2, W.split_sums(mi, q, cols["max"], 8)[0])
                s1 = max([s1] + [abs(W.split_sums(mi, q, cols[f"S1{t}[{o}]"], 8)[1]) for t in "+-"])
    print(f"largest S2 = {s2} = 2^{np.log2(float(s2)):.3f}, largest |S1| = {s1} = 2^{np.log2(float(s1)):.3f}")
    assert 1 << 51 <= s2 <= 1 << 53 and 1 << 50 <= s1 <= 1 << 53


@pytest.mark.parametrize("m", [1, 9, 16])
def test_out_of_range_words_on_the_fp64_fixed_path(F, eng, m):
    """One word >= p_j sends the whole coefficient through the cold branch that folds every limb; the result is that of the
    residues reduced modulo p_j."""
    N, k = E.N_SMALL, 3
    mi, mo = E.moduli(F, m, k, False)
    x, names, _ = E.columns(mi, mo, N, 900 + m)
    top = W.residues_from_digits(mi, [p - 1 for p in mi])
    words = lambda p: [2**64 - 1, p, p + 1, 2**63, (p >> 32) << 32]
    touched = []
    for w in range(5):
        # columns after the worst ones (first workgroup), and the last ones of the second workgroup
        one, every, in_top = (len(names) + 3 * w + i for i in range(3))
        late = N - 1 - w
        x[:, in_top] = top
        for c in (one, in_top):
            x[(w + c) % m, c] = words(mi[(w + c) % m])[w]
        for c in (every, late):
            for j in range(m):
                x[j, c] = words(mi[j])[w]
        touched += [one, every, in_top, late]
    assert len(set(touched)) == 20 and len(names) + 15 <= 256 < min(touched[3::4])
    assert sum((x[j] >= mi[j]).sum() for j in range(m)) >= 16        # ((p >> 32) << 32 is below p: a word with an empty low half)
    reduced = x % np.array(mi, dtype=np.uint64)[:, None]
    want = O.baseconv_exact(reduced, mi, mo)
    for c in touched:
        assert W.exact_reference(mi, mo, [int(v) for v in reduced[:, c]])[1] == [int(v) for v in want[:, c]]
    got = E.convert(F, eng, mi, mo, x)
    assert not _bad_columns(got, want, []), _bad_columns(got, want, [])


def test_long_grid_takes_a_second_trip(F, eng):
    mi, mo, x, names, want_worst, cols = E.long_case(F)
    got = E.convert(F, eng, mi, mo, x)
    assert not _bad_columns(got[:, :len(names)], want_worst, names)
    want = O.baseconv_exact(np.ascontiguousarray(x[:, cols]), mi, mo)
    assert (got[:, cols] == want).all()


def test_runtime_m_kernels_for_small_bases(F):
    """FHE_BC_VARIANT=0 sends m <= 16 through the runtime-m kernels (staged at N = 300, unstaged on the long grid).  The switch is read
    once per process, so a fresh child runs them and reports hashes; this process computes the expected ones."""
    want = {}
    for m in E.VARIANT0_SIZES:
        for big in (False, True):
            mi, mo, x, names, want_worst = E.small_case(F, m, E.VARIANT0_K, big)
            words = O.baseconv_exact(x, mi, mo)
            assert (words[:, :len(names)] == want_worst).all()
            want[f"m{m}-{'u64' if big else 'f64'}"] = E.sha(words)
    mi, mo, x, names, want_worst, cols = E.long_case(F)
    words = O.baseconv_exact(np.ascontiguousarray(x[:, cols]), mi, mo)
    assert (words[:, np.searchsorted(cols, np.arange(8))] == want_worst[:, :8]).all()
    want["long"] = E.sha(words)
    r = subprocess.run([sys.executable, CHILD], env=dict(os.environ, FHE_BC_VARIANT="0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert sorted(got) == sorted(want)
    assert not [c for c in want if got[c] != want[c]], [c for c in want if got[c] != want[c]]
