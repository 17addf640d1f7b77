"""ABFT-checked four-step transform (fhe_fourstep_ntt_checked / _checked_phases, fourstep_checked.hip): the words are those of
fhe_fourstep_ntt_batch and of the oracle, clean runs raise no flag, a fault between the launches or inside one raises exactly the
flag of its vector and phase, faults outside the transform raise none, and the two test hooks are one shot."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MOD, G = 998244353, 3
OK, INVALID, UNSUPPORTED = 0, 1, 3
TILES = {13: (2, 16), 14: (4, 16), 16: (16, 16), 17: (32, 32)}     # workgroups per vector of launch 1 / launch 2 (ntt_plan.hpp)


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


@pytest.fixture(scope="module")
def O():
    from oracle import cport
    return cport


@pytest.fixture(scope="module")
def L():
    from fhe_reliability_gpu_amd._lib import lib
    return lib


def _prime(O, logn, bits):
    """(q, g) with N | q - 1 and g a quadratic non-residue, so that g^((q-1)/N) has order exactly N"""
    q = O.gen_primes(1 << logn, bits, 1)[0]
    return q, next(c for c in range(2, 1000) if pow(c, (q - 1) // 2, q) == q - 1)


_CASES = {}


def _case(F, eng, O, n1, n2, mod=MOD, g=G, n_vec=3):
    """plan, input, oracle output and the unchecked call's output for one shape -- computed once, shared, never modified"""
    key = (n1, n2, mod, n_vec)
    if key not in _CASES:
        N = n1 * n2
        rng = np.random.default_rng(N % 1000 + mod % 97 + n_vec)
        x = rng.integers(0, mod, (n_vec, N), dtype=np.uint64)
        x[n_vec - 1, : N // 4] = mod - 1
        want = np.stack([O.four_step_ntt(v, n1, n2, mod, g) for v in x])
        fs = F.FourStep(eng, n1, n2, mod, g)
        src, dst = eng.upload(x), eng.alloc(x.size)
        fs.ntt(src, dst, n_vec)
        plain = dst.download().reshape(x.shape)
        _CASES[key] = (fs, x, want, plain)
    return _CASES[key]


def _weights(O, n1, n2, mod, g):
    N, lp = n1 * n2, (n1 * n2).bit_length() - 1 >> 1
    v = np.array([((i % (1 << lp)) + 1 + (i >> lp) + 1) % mod for i in range(N)], dtype=np.uint64)
    return O.four_step_ntt(v, n1, n2, mod, g), v


def _dot(w, x, q):
    return sum(int(a) * int(b) for a, b in zip(w, x)) % q


SHAPES = [(4, 4), (4, 8), (64, 64), (64, 128), (128, 128), (256, 256), (512, 256)]


@pytest.mark.parametrize("n1,n2", SHAPES)
def test_clean_runs_match_oracle_and_unchecked_call(F, eng, O, n1, n2):
    fs, x, want, plain = _case(F, eng, O, n1, n2)
    n_vec, N = x.shape
    assert (plain == want).all()
    for inplace in (False, True):
        src = eng.upload(x)
        dst = src if inplace else eng.alloc(x.size)
        flags = fs.ntt_checked(src, dst, n_vec)
        got = dst.download().reshape(x.shape)
        assert (got == want).all() and (got == plain).all()
        assert flags.tolist() == [0] * n_vec
        if N >= 1 << 13:
            src = eng.upload(x)
            dst = src if inplace else eng.alloc(x.size)
            flags = fs.ntt_checked_phases(src, dst, n_vec)
            assert (dst.download().reshape(x.shape) == plain).all()
            assert not flags.any() and flags.shape == (n_vec, 3)


@pytest.mark.parametrize("bits", [50, 61])
def test_clean_runs_with_large_primes(F, eng, O, bits):
    q, g = _prime(O, 14, bits)
    fs, x, want, plain = _case(F, eng, O, 128, 128, q, g)
    assert (plain == want).all()
    src, dst = eng.upload(x), eng.alloc(x.size)
    assert not fs.ntt_checked(src, dst, 3).any()
    assert (dst.download().reshape(x.shape) == want).all()
    assert not fs.ntt_checked_phases(src, src, 3).any()
    assert (src.download().reshape(x.shape) == want).all()


@pytest.mark.parametrize("n1,n2", [(32, 32), (128, 128)])
def test_an_out_of_range_input_word_stays_clean(F, eng, O, n1, n2):
    fs, x, want, plain = _case(F, eng, O, n1, n2)
    y = x.copy()
    y[1, 7] = 2**64 - 5
    src, ref, dst = eng.upload(y), eng.alloc(y.size), eng.alloc(y.size)
    fs.ntt(src, ref, 3)
    assert not fs.ntt_checked(src, dst, 3).any()
    got = dst.download().reshape(y.shape)
    assert (got == ref.download().reshape(y.shape)).all()
    y[1, 7] = (2**64 - 5) % MOD
    assert (got[1] == O.four_step_ntt(y[1], n1, n2, MOD, G)).all()


@pytest.mark.parametrize("n1,n2", [(32, 32), (128, 128)])
def test_checksum_sides_equal_the_host_dot_products(F, eng, O, n1, n2):
    fs, x, want, plain = _case(F, eng, O, n1, n2)
    u, v = _weights(O, n1, n2, MOD, G)
    s0 = fs.checksum(eng.upload(x), 0, 3)
    s1 = fs.checksum(eng.upload(want), 1, 3)
    assert s0.tolist() == [_dot(u, r, MOD) for r in x]
    assert s1.tolist() == [_dot(v, r, MOD) for r in want]
    assert s0.tolist() == s1.tolist()


@pytest.mark.parametrize("n1,n2", [(64, 128), (128, 128), (256, 256), (512, 256)])
def test_fault_between_the_launches(F, eng, O, L, n1, n2):
    fs, x, want, plain = _case(F, eng, O, n1, n2)
    n_vec, N = x.shape
    # (hand-off words are FP64 bit patterns of integers here: the sign and the two top mantissa bits keep them integers)
    for vec, word, bit in ((0, 0, 63), (2, N - 1, 51), (1, N // 3, 50)):
        src, dst = eng.upload(x), eng.alloc(x.size)
        assert L.fhe_ctx_inject_fault(eng._h, vec * N + word, bit) == OK
        flags = fs.ntt_checked(src, dst, n_vec)
        assert flags.tolist() == [int(i == vec) for i in range(n_vec)], (vec, word, bit, flags)
        bad = (dst.download().reshape(x.shape) != plain).any(axis=1)
        assert bad.tolist() == [i == vec for i in range(n_vec)]
        assert L.fhe_ctx_inject_fault(eng._h, vec * N + word, bit) == OK
        flags = fs.ntt_checked_phases(src, dst, n_vec)
        want_f = np.zeros((n_vec, 3), dtype=np.uint32)
        want_f[vec, 1] = 1
        assert (flags == want_f).all(), (vec, word, bit, flags)
        bad = (dst.download().reshape(x.shape) != plain).any(axis=1)
        assert bad.tolist() == [i == vec for i in range(n_vec)]


def _row_word(row, g):
    """LDS word of point g of local row `row` in launch 1's image (rows of 256 points, 2 words of padding after every 16)"""
    return row * 288 + g + (g >> 4) * 2


def _col_word(pt, col):
    """LDS word of point pt of column col in launch 2's image (16 columns, 16 words of padding after every 16 points)"""
    return pt * 16 + col + (pt >> 4) * 16


@pytest.mark.parametrize("logn,path", [(14, 0), (14, 1), (16, 0)])
def test_fault_inside_a_launch(F, eng, O, L, logn, path):
    n1 = n2 = 1 << (logn // 2)
    mod, g = (MOD, G) if path == 0 else _prime(O, logn, 61)
    fs, x, want, plain = _case(F, eng, O, n1, n2, mod, g)
    n_vec, N = x.shape
    t1, t2 = TILES[logn]
    col_pts = N // 256
    bits = (63, 51, 50) if path == 0 else (0, 17, 40)      # integer path: low bits keep the word inside its lazy range
    for p, tiles in ((0, t1), (1, t2)):
        last = n_vec * tiles - 1
        if p == 0:
            spots = [(0, _row_word(0, 0)), (1, _row_word(15, 255)), (last // 2, _row_word(7, 100)), (last // 2 + 1, _row_word(3, 16)),
                     (last - 1, _row_word(9, 31)), (last, _row_word(12, 200))]
        else:
            spots = [(0, _col_word(0, 0)), (1, _col_word(col_pts - 1, 15)), (last // 2, _col_word(col_pts // 2, 7)), (last // 2 + 1, _col_word(17, 3)),
                     (last - 1, _col_word(33, 12)), (last, _col_word(5, 9))]
        for i, (wg, word) in enumerate(spots):
            bit = bits[i % 3]
            src, dst = eng.upload(x), eng.alloc(x.size)
            assert L.fhe_ctx_inject_fault_in_pass(eng._h, p, wg, word, bit) == OK
            flags = fs.ntt_checked_phases(src, dst, n_vec)
            want_f = np.zeros((n_vec, 3), dtype=np.uint32)
            want_f[wg // tiles, 2 * p] = 1
            assert (flags == want_f).all(), (p, wg, word, bit, flags)
    src, dst = eng.upload(x), eng.alloc(x.size)
    assert not fs.ntt_checked_phases(src, dst, n_vec).any()          # the hook is one shot
    assert (dst.download().reshape(x.shape) == plain).all()


def test_faults_outside_the_transform_raise_no_flag(F, eng, O, L):
    fs, x, want, plain = _case(F, eng, O, 128, 128)
    n_vec, N = x.shape
    src, dst = eng.upload(x), eng.alloc(x.size)
    assert L.fhe_flip_bit(eng._h, src.ptr, 1 * N + 99, 5, None) == OK       # a fault already in the input
    assert not fs.ntt_checked(src, dst, n_vec).any()
    assert not fs.ntt_checked_phases(src, dst, n_vec).any()
    bad = (dst.download().reshape(x.shape) != plain).any(axis=1)
    assert bad.tolist() == [False, True, False]


def test_hooks_are_consumed_and_refused_where_they_have_no_point(F, eng, O, L):
    fs, x, want, plain = _case(F, eng, O, 128, 128)
    small, xs, _, plain_s = _case(F, eng, O, 32, 32)
    n_vec, N = x.shape
    src, dst = eng.upload(x), eng.alloc(x.size)
    ssrc, sdst = eng.upload(xs), eng.alloc(xs.size)
    flags = eng.alloc(8)
    # between-launch hook before a single-launch size: refused, and gone afterwards
    assert L.fhe_ctx_inject_fault(eng._h, 5, 3) == OK
    assert L.fhe_fourstep_ntt_checked(eng._h, sdst.ptr, ssrc.ptr, small._h, 3, flags.ptr, None) == UNSUPPORTED
    assert not fs.ntt_checked(src, dst, n_vec).any()
    assert (dst.download().reshape(x.shape) == plain).all()
    # in-pass hook on the whole-transform call: refused, and gone afterwards
    assert L.fhe_ctx_inject_fault_in_pass(eng._h, 0, 0, 0, 63) == OK
    assert L.fhe_fourstep_ntt_checked(eng._h, dst.ptr, src.ptr, fs._h, n_vec, flags.ptr, None) == UNSUPPORTED
    assert not fs.ntt_checked_phases(src, dst, n_vec).any()
    # an index outside the call's window
    assert L.fhe_ctx_inject_fault(eng._h, n_vec * N, 3) == OK
    assert L.fhe_fourstep_ntt_checked(eng._h, dst.ptr, src.ptr, fs._h, n_vec, flags.ptr, None) == INVALID
    assert L.fhe_ctx_inject_fault_in_pass(eng._h, 1, n_vec * 16, 0, 3) == OK
    assert L.fhe_fourstep_ntt_checked_phases(eng._h, dst.ptr, src.ptr, fs._h, n_vec, flags.ptr, None) == INVALID
    # after a consumed hook the next call is clean
    assert L.fhe_ctx_inject_fault(eng._h, 17, 63) == OK
    assert fs.ntt_checked(src, dst, n_vec).tolist() == [1, 0, 0]
    assert not fs.ntt_checked(src, dst, n_vec).any()
    assert (dst.download().reshape(x.shape) == plain).all()
    assert not small.ntt_checked(ssrc, sdst, 3).any()
    assert (sdst.download().reshape(xs.shape) == plain_s).all()


@pytest.fixture
def small_chunks(eng):
    """1 MiB sub-batches with no lower bound on the batch size, so that small inputs are cut"""
    eng.set_option("ntt_chunk_mib", 1)
    eng.set_option("ntt_chunk_floor_mib", 0)
    yield
    eng.sync()
    eng.check()
    for k, v in (("ntt_chunk_mib", 96), ("ntt_chunk_floor_mib", 192), ("ntt_split", -1), ("ntt_pingpong", -1), ("ntt_stream", -1)):
        eng.set_option(k, v)


@pytest.mark.parametrize("option", ["ntt_split", "ntt_pingpong", "ntt_stream"])
@pytest.mark.parametrize("value", [0, 1])
def test_forced_cut(F, eng, O, L, small_chunks, option, value):
    fs, x, want, plain = _case(F, eng, O, 128, 128, n_vec=24)
    n_vec, N = x.shape
    assert (plain == want).all()
    eng.set_option(option, value)
    src, dst = eng.upload(x), eng.alloc(x.size)
    assert not fs.ntt_checked(src, dst, n_vec).any()
    assert (dst.download().reshape(x.shape) == want).all()
    assert not fs.ntt_checked_phases(src, src, n_vec).any()
    assert (src.download().reshape(x.shape) == want).all()
    # with the hook armed the batch runs whole: the index addresses the hand-off buffer of all 24 vectors
    src = eng.upload(x)
    assert L.fhe_ctx_inject_fault(eng._h, 20 * N + 4321, 51) == OK
    flags = fs.ntt_checked_phases(src, dst, n_vec)
    want_f = np.zeros((n_vec, 3), dtype=np.uint32)
    want_f[20, 1] = 1
    assert (flags == want_f).all()
    bad = (dst.download().reshape(x.shape) != want).any(axis=1)
    assert bad.tolist() == [i == 20 for i in range(n_vec)]


def test_statuses(F, eng, O, L):
    small, xs, _, _ = _case(F, eng, O, 32, 32)
    ssrc, sdst = eng.upload(xs), eng.alloc(xs.size)
    pattern = np.full(8, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    flags = eng.upload(pattern)
    assert L.fhe_fourstep_ntt_checked_phases(eng._h, sdst.ptr, ssrc.ptr, small._h, 3, flags.ptr, None) == UNSUPPORTED      # phases below 2^13
    assert L.fhe_fourstep_ntt_checked(eng._h, sdst.ptr, ssrc.ptr, small._h, 0, flags.ptr, None) == OK                      # n_vec = 0
    assert (flags.download() == pattern).all()
    assert L.fhe_fourstep_ntt_checked(eng._h, sdst.ptr, ssrc.ptr, small._h, 3, None, None) == INVALID                      # null flags
    big = F.FourStep(eng, 2048, 1024)                   # N = 2^21: created only, nothing of that size is run
    for call in (L.fhe_fourstep_ntt_checked, L.fhe_fourstep_ntt_checked_phases):
        assert call(eng._h, sdst.ptr, ssrc.ptr, big._h, 1, flags.ptr, None) == UNSUPPORTED
    assert L.fhe_fourstep_prepare_checked(eng._h, big._h, None) == UNSUPPORTED
    big.close()
    assert (flags.download() == pattern).all()


@pytest.mark.parametrize("N", [16, 1 << 14])
def test_reference_named_function(F, eng, O, N):
    rng = np.random.default_rng(N)
    a = rng.integers(0, MOD, N, dtype=np.uint64)
    y, checks = F.four_step_with_protection_vector([int(v) for v in a], N, MOD, G, eng=eng)
    n1 = 1 << ((N.bit_length() - 1) // 2)
    assert y == [int(v) for v in O.four_step_ntt(a, n1, N // n1, MOD, G)]
    assert set(checks) == ({"transform"} if N < 1 << 13 else {"stage1", "handoff", "stage2"})
    assert all(c["ok"] is True for c in checks.values())
