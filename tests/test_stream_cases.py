"""The designed products of tests/helpers/stream_cases.py do what they were designed for (no GPU): for every modulus the GPU tests
use, barrett128()'s quotient estimate is one short on every lifted pair and on at least half of the canonical pairs -- or, for the
moduli where canonical words cannot get there, on none, and the test names those moduli.  The estimate is never two short.

The closed form.  With rho = 2^128 mod q, x floor(2^128 / q) / 2^128 = x / q - x rho / (q 2^128), and the nested floors of the
64-bit words give the floor of exactly this number (the dropped low word of lo * r0 cannot carry into it).  For x = k q + s the
estimate is therefore k - ceil((x rho - s 2^128) / (q 2^128)) when that is positive: one short exactly when s 2^128 < x rho, and
never two, since x rho < q 2^128.  Canonical words reach it only when (q - 1)^2 rho > 2^128."""
import numpy as np
import pytest

from helpers import stream_cases as S

# (N, prime sizes) of every table set of tests/test_gpu_stream_products.py and tests/test_gpu_long_grids.py
TABLES = [(2, [50, 61, 30, 61, 50]), (1 << 10, [50, 61, 30, 61, 50]), (1 << 12, [50, 61, 50]), (1 << 14, [50, 61, 50, 61, 50, 61, 50]),
          (1 << 16, [50, 61] * 48 + [50])]
N_PAIRS = 200


@pytest.fixture(scope="module")
def moduli():
    import fhe_reliability_gpu_amd as F
    qs = []
    for N, bits in TABLES:
        for q in F.create_moduli(N, bits):
            if q not in qs:
                qs.append(q)
    return qs


def _closed_form(x, q):
    rho = (1 << 128) % q
    return 1 if (x % q) << 128 < x * rho else 0


def _reachable(q):
    return (q - 1) ** 2 * ((1 << 128) % q) > 1 << 128


def test_the_restated_estimate_is_the_floor_of_the_real_quotient_estimate(moduli):
    rng = np.random.default_rng(1)
    for q in moduli[:12] + [(1 << 61) - 1, (1 << 60) + 33]:
        ratio = (1 << 128) // q
        for _ in range(300):
            x = int(rng.integers(0, S.M64, endpoint=True, dtype=np.uint64)) << 64 | int(rng.integers(0, S.M64, endpoint=True, dtype=np.uint64))
            x >>= int(rng.integers(0, 70))
            assert S.barrett_qhat(x, q) == (x * ratio >> 128) & S.M64
            assert S.barrett_shortfall(x, q) == _closed_form(x, q)
            assert S.barrett128(x, q) == x % q


def test_every_lifted_pair_is_one_short(moduli):
    rng = np.random.default_rng(2)
    assert {q.bit_length() for q in moduli} == {30, 50, 61}
    for q in moduli:
        pairs = S.small_residue_pairs(q, N_PAIRS, rng, lift=True)
        assert len(pairs) == N_PAIRS
        exact = [a * b for a, b in pairs if a * b in (q, 2 * q, q * (q - 1))]
        assert len(exact) == 3
        for a, b in pairs:
            assert a <= S.M64 and b <= S.M64 and a * b % q in (0, 1, 2, 3)
            assert a + q > S.M64 or a * b in exact, "not the largest word of its class"
            assert S.barrett_shortfall(a * b, q) == 1, (q, a, b)
            assert S.barrett128(a * b, q) == a * b % q


def test_canonical_pairs_are_one_short_wherever_canonical_words_can_be(moduli):
    rng = np.random.default_rng(3)
    unreachable = []
    for q in moduli:
        pairs = S.small_residue_pairs(q, N_PAIRS, rng)
        assert pairs[:2] == [(q - 1, q - 1), (1, 1)]
        assert all(q // 2 <= a < q and 0 < b < q for a, b in pairs[2:])
        assert [a * b % q for a, b in pairs[2:8]] == [1, 2, 3, 1, 2, 3]
        short = [S.barrett_shortfall(a * b, q) for a, b in pairs]
        assert set(short) <= {0, 1}, (q, "a shortfall of 2 would be a third class of pairs")
        assert short == [_closed_form(a * b, q) for a, b in pairs]
        if _reachable(q):
            assert 2 * sum(short) >= len(pairs), (q, sum(short))
            assert short[0] == 1                      # (q - 1)^2: the one pair the older tests have
        else:
            unreachable.append(q)
            assert not any(short), q
    # no modulus is dropped silently: the ones canonical words cannot bring to the subtraction are exactly the 30-bit primes
    assert unreachable and all(q.bit_length() == 30 for q in unreachable), unreachable
    assert sorted(unreachable) == sorted(q for q in moduli if q.bit_length() == 30)


def test_special_primes_behave_as_the_closed_form_says():
    """2^61 - 1 has 2^128 mod q = 64: no canonical product is short, every lifted one is.  2^60 + 33 (not a create_moduli prime either)
    is reachable.  Neither can come out of create_moduli at the sizes used, so they are not run on the GPU."""
    rng = np.random.default_rng(4)
    m61 = (1 << 61) - 1
    assert not _reachable(m61)
    assert not any(S.barrett_shortfall(a * b, m61) for a, b in S.small_residue_pairs(m61, N_PAIRS, rng))
    assert all(S.barrett_shortfall(a * b, m61) == 1 for a, b in S.small_residue_pairs(m61, N_PAIRS, rng, lift=True))
    q = (1 << 60) + 33
    assert _reachable(q)
    assert all(S.barrett_shortfall(a * b, q) == 1 for a, b in S.residue_pairs(q, N_PAIRS, rng, (1, 2, 3)))


def test_fp64_edge_pairs_land_on_both_sides_of_zero(moduli):
    rng = np.random.default_rng(5)
    for q in [q for q in moduli if q.bit_length() == 50][:6]:
        pairs = S.fp64_edge_pairs(q, 50, rng)
        assert [a * b % q for a, b in pairs[:5]] == [1, q - 1, 2, q - 2, 3]
        assert all(q // 2 <= a < q and 0 < b < q for a, b in pairs)


def test_the_long_cases_pass_their_caps_with_a_partial_last_trip():
    """the table says which case reaches which trip (nothing here reads a launcher)"""
    want_trips = {"pointwise 3 x 256": 2, "modmul 3 x 512": 2, "modmul non-temporal 3 x 683": 3, "tensor 97 limbs": 2, "columns": 2, "hadamard": 2,
                  "seal 12285 rows": 2, "seal two chunks": 1, "repair 3073 rows": 2}
    assert set(want_trips) == set(S.LONG_CASES)
    for case, (launchers, elements) in S.LONG_CASES.items():
        for name in launchers:
            n, partial = S.trips(name, elements)
            if S.stride(name) is None:
                continue
            assert n == want_trips[case], (case, name, n)
            assert partial, (case, name)
    assert S.LONG_CASES["modmul non-temporal 3 x 683"][1] == 8392704 > 8388608
    rng = np.random.default_rng(6)
    cols = S.sample_columns(4096, 511 * 4096, 1 << 21, rng)
    assert len(cols) == 64 and cols[0] == 0 and cols[-1] == 4095 and len(set(cols.tolist())) == 64
    cols = S.sample_columns(4096, 512 * 4096, 1 << 21, rng)                  # the row that begins the second trip
    assert cols[0] == 0
    cols = S.sample_columns(1 << 16, 63 << 16, 1 << 22, rng)                 # the second trip begins behind this row's last word
    assert cols[-1] == (1 << 16) - 1
    cols = S.sample_columns(1572867, 0, 1 << 20, rng)
    assert {(1 << 20) - 1, 1 << 20, 1572866} <= set(cols.tolist())
