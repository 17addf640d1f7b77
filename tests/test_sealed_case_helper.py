"""The functions of tests/helpers/sealed_case.py that the sealed GPU tests' assertions rest on, on hand-made inputs -- without a GPU."""
import numpy as np

from helpers.sealed_case import P, HostCase, PLANS, case_cache, flat, py_seals, py_seals_and_locator, raised, safe_coeff

FLAGS = {"key": np.array([[0, 1], [0, 2]]), "b0": None, "checked": {"tail": np.array([0, 0, 3]), "mac": np.zeros((2, 2), dtype=np.uint32), "skipped": None},
         "a0": np.array([4, 0])}


def test_raised_names_every_nonzero_word_by_its_flat_unit_in_the_dictionarys_order():
    assert raised(FLAGS) == [("key", 1), ("key", 3), ("checked.tail", 2), ("a0", 0)]
    assert raised({"a0": np.zeros(3), "b0": None, "checked": {"tail": np.zeros((2, 2))}}) == []
    assert raised({"rot_in": [{"c0": np.array([0, 1])}, {"c0": np.array([1, 0])}]}) == [("rot_in[0].c0", 1), ("rot_in[1].c0", 0)]


def test_flat_lists_every_word_sorted_by_name_and_leaves_none_out():
    assert flat(FLAGS) == [("a0", [4, 0]), ("checked.mac", [0, 0, 0, 0]), ("checked.tail", [0, 0, 3]), ("key", [0, 1, 0, 2])]
    assert flat({"rot": [{"b": np.array([1])}, {"a": np.array([[2], [3]])}]}) == [("rot[0].b", [1]), ("rot[1].a", [2, 3])]
    # the order is the names', not the dictionary's: two dictionaries built in another order compare equal
    assert flat({"x": np.array([1]), "a": np.array([2])}) == flat({"a": np.array([2]), "x": np.array([1])})
    assert flat({"a": np.array([0, 1])}) != flat({"a": np.array([1, 0])})


def test_py_seals_are_the_plain_and_the_index_weighted_sum_modulo_the_mersenne_prime():
    x = np.array([[[5, 7, 11], [P - 1, 2, 0]]], dtype=np.uint64)      # [1][2][3]: rows are the last axis
    assert py_seals(x) == [[23, 5 + 2 * 7 + 3 * 11], [1, 3]]           # (P - 1) + 2 = 1, (P - 1) + 2 * 2 = 3 modulo P
    assert py_seals_and_locator(x) == [[23, 52, 5 + 4 * 7 + 9 * 11], [1, 3, 7]]
    big = np.full((1, 4), (1 << 63) + 1, dtype=np.uint64)              # sums that pass 2^64: Python integers, no wrap
    assert py_seals(big) == [[4 * ((1 << 63) + 1) % P, 10 * ((1 << 63) + 1) % P]]


def test_safe_coeff_passes_over_a_word_that_a_flipped_bit_would_carry_to_q():
    q = 1000
    row = np.array([1, 990, 984, 983, 5], dtype=np.uint64)
    assert safe_coeff(row, q, 1) == 3              # 990 and 984 are not below q - 16
    assert safe_coeff(row, q, 0) == 0 and safe_coeff(row, q, 4) == 4
    assert safe_coeff(row, q, 1, room=64) == 4     # 983 is not below q - 64


def test_case_cache_makes_each_case_once():
    made = []
    get = case_cache(lambda key: made.append(key) or [key])
    assert get("A") is get("A") and get("B") == ["B"] and made == ["A", "B"]


def test_the_host_draw_is_seeded_in_range_and_in_the_order_operands_then_key():
    import fhe_reliability_gpu_amd as F
    c = HostCase(F, PLANS["A"], seed=3, margin=16, n_ops=2)
    assert (c.logn, c.L, c.K, c.dnum, c.N, c.M) == (10, 4, 2, 2, 1024, 6)
    assert [v.shape for v in c.ops] == [(4, 1024)] * 2 and c.key.shape == (2, 2, 6, 1024)
    rng = np.random.default_rng(3)
    want = [rng.integers(16, q - 16, c.N, dtype=np.uint64) for _ in range(2) for q in c.qs[:c.L]]
    want += [rng.integers(16, q - 16, c.N, dtype=np.uint64) for _ in range(c.dnum * 2) for q in c.qs]
    assert (np.concatenate([v.reshape(-1) for v in c.ops] + [c.key.reshape(-1)]) == np.concatenate(want)).all()
