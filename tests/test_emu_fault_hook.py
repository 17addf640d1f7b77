"""The one-shot test hooks of the checked and sealed calls on the CPU (tests/emu/emu_fault_hook.cpp compiles fault_hook.hpp, the
records the context stores and the code every fhe_ctx_inject_fault_* setter and every checked or sealed call shares): what the
setters accept, refuse and store equals a table written here from the rules of include/fhe_mi355x.h, take() hands a hook out
once, the check-record builder arms exactly the launch whose flags hold the fault's unit, and a sealed hook's word is inside a
call exactly when its row and word are -- without a GPU."""
import ctypes as C
import itertools

import pytest

from helpers.emu_build import build_emu

Rec6, Rec5, Rec4 = C.c_longlong * 6, C.c_longlong * 5, C.c_longlong * 4

T = "transform"          # a transform stage: one point between its two launches, `point` ignored and stored as 0
GAL_AT_INDEX = 1         # the Galois permutation's points are 0 (the word) and 1 (the source index)
# include/fhe_mi355x.h, per setter: the highest point of every stage
RULES = {
    "keyswitch": [T, 3, T, 3, T, 3, T, 3],                              # fhe_ctx_inject_fault_keyswitch: stages 0, 2, 4, 6 transforms
    "rescale": [T, 3, T, 3],                                            # fhe_ctx_inject_fault_rescale: stages 0, 2 transforms
    "rotate_hoisted": [T, 3, T, 3, T, 3, T, 3, GAL_AT_INDEX],           # the key switch's stages, stage 8 the Galois permutation's points
    "bsgs": [3, 3],                                                     # fhe_ctx_inject_fault_bsgs: no transform stage
}
FAMILY = {name: i for i, name in enumerate(RULES)}
DISARMED = (0, -1, 0, 0, 0, 0)             # (block, stage, point, unit, coeff, bit)
SENTINEL = (2, 1, 2, 9, 11, 13)            # an armed hook that every family's rules accept


@pytest.fixture(scope="module")
def emu():
    # variation: no -ffp-contract=off -- emu_fault_hook.cpp does integer work only, and the flags stay as they have always been
    L = build_emu("libemu_fault_hook.so", ["emu_fault_hook.cpp"], ("fault_hook.hpp", "galois_check.hpp", "modarith.hpp"), flags=("-O2", "-std=c++17"))
    ll, i = C.c_longlong, C.c_int
    L.emu_hook_stages.argtypes = [i]
    L.emu_hook_arm.argtypes = [i, Rec6, i, i, i, i, ll, i, Rec6]
    L.emu_hook_take_twice.argtypes = [i, i, i, i, i, ll, i, Rec6, Rec6, Rec6]
    L.emu_point_arm.argtypes = [i, Rec4, i, i, ll, i, Rec4]
    L.emu_point_take_twice.argtypes = [i, i, i, ll, i, Rec4, Rec4, Rec4]
    L.emu_seal_arm.argtypes = [i, Rec5, i, i, i, ll, i, Rec5]
    L.emu_seal_take_twice.argtypes = [i, i, i, i, ll, i, Rec5, Rec5, Rec5]
    L.emu_seal_inside.argtypes = [i, ll, C.c_ulonglong, i]
    L.emu_bc_check.argtypes = [Rec6, i, i, i, i, i, C.c_longlong * 3, C.POINTER(C.c_uint64)]
    return L


def expected(rules, before, block, stage, point, unit, coeff, bit):
    """(accepted, hook afterwards) by the header's rules"""
    if stage < 0:                                                   # "stage < 0 clears it"
        return True, (before[0], -1) + tuple(before[2:])
    if stage >= len(rules) or block < 0 or unit < 0 or coeff < 0 or not 0 <= bit <= 63:
        return False, before
    if rules[stage] == T:
        return True, (block, stage, 0, unit, coeff, bit)
    if not 0 <= point <= rules[stage]:
        return False, before
    return True, (block, stage, point, unit, coeff, bit)


@pytest.mark.parametrize("name", list(RULES))
def test_setter_core_accepts_refuses_and_stores_by_the_headers_rules(emu, name):
    rules, fam = RULES[name], FAMILY[name]
    assert emu.emu_hook_stages(fam) == len(rules)
    n = accepted = 0
    for before in (DISARMED, SENTINEL):
        grid = itertools.product((-1, 0, 3), range(-1, len(rules) + 1), range(-1, 5), (-1, 0, 5), (-1, 0, 7), (-1, 0, 17, 63, 64))
        for block, stage, point, unit, coeff, bit in grid:
            stored = Rec6()
            got = emu.emu_hook_arm(fam, Rec6(*before), block, stage, point, unit, coeff, bit, stored)
            want_ok, want = expected(rules, before, block, stage, point, unit, coeff, bit)
            assert got == int(want_ok), (name, before, block, stage, point, unit, coeff, bit)
            assert tuple(stored)[1] == want[1], (name, before, block, stage, point, unit, coeff, bit)
            if want[1] >= 0:                                        # (a disarmed hook's other fields mean nothing)
                assert tuple(stored) == want, (name, before, block, stage, point, unit, coeff, bit)
            n += 1
            accepted += got
    assert n == 2 * 3 * (len(rules) + 2) * 6 * 3 * 3 * 5
    # per accepted stage 2 blocks x 2 units x 2 coefficients x 3 bits, times 6 points on a transform stage and the stage's own
    # number elsewhere; stage -1 accepts all 3 * 6 * 3 * 3 * 5 combinations
    want_accepted = 2 * (sum(24 * (6 if r == T else r + 1) for r in rules) + 3 * 6 * 3 * 3 * 5)
    assert accepted == want_accepted


def test_unknown_family_and_families_differ_where_the_header_says_so(emu):
    assert emu.emu_hook_stages(4) == -1 and emu.emu_hook_stages(-1) == -1
    arm = lambda name, stage, point: emu.emu_hook_arm(FAMILY[name], Rec6(*DISARMED), 0, stage, point, 0, 0, 0, Rec6())
    assert arm("keyswitch", 7, 3) == 1 and arm("keyswitch", 8, 0) == 0
    assert arm("rescale", 3, 3) == 1 and arm("rescale", 4, 0) == 0
    assert arm("rotate_hoisted", 8, GAL_AT_INDEX) == 1 and arm("rotate_hoisted", 8, 2) == 0 and arm("rotate_hoisted", 9, 0) == 0
    assert arm("bsgs", 0, -1) == 0 and arm("bsgs", 1, 3) == 1 and arm("bsgs", 2, 0) == 0      # BSGS has no transform stage


@pytest.mark.parametrize("name", list(RULES))
def test_take_returns_the_armed_record_once(emu, name):
    rules, fam = RULES[name], FAMILY[name]
    for stage in range(len(rules)):
        first, second, stored = Rec6(), Rec6(), Rec6()
        assert emu.emu_hook_take_twice(fam, 3, stage, 1, 6, 21, 40, first, second, stored) == 1
        assert tuple(first) == (3, stage, 0 if rules[stage] == T else 1, 6, 21, 40)
        assert second[1] == -1 and stored[1] == -1
    # a refused setter leaves nothing to take
    first, second, stored = Rec6(), Rec6(), Rec6()
    assert emu.emu_hook_take_twice(fam, 0, len(rules), 0, 0, 0, 0, first, second, stored) == 0
    assert first[1] == -1 and second[1] == -1 and stored[1] == -1


def test_hooks_of_one_step(emu):
    """pointwise, polynomial product and base conversion (points 0-3), Galois permutation (points 0-1): point < 0 clears"""
    for max_point in (3, GAL_AT_INDEX):
        for before in ((-1, 0, 0, 0), (1, 4, 5, 6)):
            for point, unit, coeff, bit in itertools.product(range(-2, 6), (-1, 0, 5), (-1, 0, 7), (-1, 0, 17, 63, 64)):
                stored = Rec4()
                got = emu.emu_point_arm(max_point, Rec4(*before), point, unit, coeff, bit, stored)
                if point < 0:
                    assert got == 1 and stored[0] == -1
                elif point > max_point or unit < 0 or coeff < 0 or not 0 <= bit <= 63:
                    assert got == 0 and tuple(stored) == before
                else:
                    assert got == 1 and tuple(stored) == (point, unit, coeff, bit)
        first, second, stored = Rec4(), Rec4(), Rec4()
        assert emu.emu_point_take_twice(max_point, max_point, 2, 1 << 40, 63, first, second, stored) == 1
        assert tuple(first) == (max_point, 2, 1 << 40, 63) and second[0] == -1 and stored[0] == -1


def test_check_record_builder(emu):
    def build(rec, at_block, at_stage, window=None):
        out, mask = (C.c_longlong * 3)(), C.c_uint64()
        u0, u1 = window or (0, 0)
        assert emu.emu_bc_check(Rec6(*rec), at_block, at_stage, int(window is not None), u0, u1, out, C.byref(mask)) == 1, "the caller's flags pointer"
        return tuple(out) + (mask.value,)

    clean = (-1, 0, 0, 0)
    # disarmed, and armed for another stage or block
    assert build(DISARMED, 0, 0) == clean and build(DISARMED, 0, 3, (0, 8)) == clean
    rec = (1, 3, 2, 10, 123456, 63)         # block 1, stage 3, point 2, unit 10, coefficient 123456, bit 63
    assert build(rec, 1, 2) == clean and build(rec, 0, 3) == clean
    # armed, the default window
    assert build(rec, 1, 3) == (2, 10, 123456, 1 << 63)
    # armed, unit windows: below, inside (rebased by u0), the ends, above
    assert build(rec, 1, 3, (0, 10)) == clean
    assert build(rec, 1, 3, (10, 11)) == (2, 0, 123456, 1 << 63)
    assert build(rec, 1, 3, (4, 12)) == (2, 6, 123456, 1 << 63)
    assert build(rec, 1, 3, (11, 20)) == clean
    for bit in (0, 1, 31, 32, 63):
        assert build((0, 1, 0, 0, 0, bit), 0, 1) == (0, 0, 0, 1 << bit)


# ---- the hooks of the sealed calls.  include/fhe_mi355x.h, per setter: its arguments before (coeff, bit) with the one that disarms
# when negative (the selector) first, the selector's highest value (None: the setter has no upper bound, the call that takes the
# hook checks it), and where the context's record (sel, idx, row) keeps them
INT_MAX = 2**31 - 1
SEALED = {
    # fhe_ctx_inject_fault_bsgs_sealed(g, b, limb, coeff, bit): "g < 0 clears"
    "bsgs_sealed": dict(max=None, others=2, record=lambda g, b, limb: (g, b, limb)),
    # fhe_ctx_inject_fault_tensor_sealed(operand, row, coeff, bit): "operand 0..3 = a0, a1, b0, b1, negative clears"
    "tensor_sealed": dict(max=3, others=1, record=lambda op, row: (op, 0, row)),
    # fhe_ctx_inject_fault_keyswitch_sealed(key_row, coeff, bit): "negative clears"; the key row is the row of the word
    "keyswitch_sealed": dict(max=None, others=0, record=lambda key_row: (key_row, 0, key_row)),
    # fhe_ctx_inject_fault_galois_sealed(rot, point, row, coeff, bit): "a negative point clears", points 0 and 1; others = (rot, row)
    "galois_sealed": dict(max=GAL_AT_INDEX, others=2, record=lambda point, rot, row: (point, rot, row)),
    # fhe_ctx_inject_fault_ntt_sealed(row, coeff, bit): "a negative row clears"; the selector is the row of the word
    "ntt_sealed": dict(max=None, others=0, record=lambda row: (row, 0, row)),
}
SEAL_DISARMED = (-1, 0, 0, 0, 0)           # (sel, idx, row, coeff, bit)
SEAL_SENTINEL = (1, 4, 6, 11, 13)          # an armed hook that every setter's rules accept


def seal_expected(spec, before, sel, others, coeff, bit):
    """(accepted, hook afterwards) by the header's rules"""
    if sel < 0:                                                     # disarms "whatever the other arguments hold"
        return True, (-1,) + tuple(before[1:])
    if (spec["max"] is not None and sel > spec["max"]) or any(o < 0 for o in others) or coeff < 0 or not 0 <= bit <= 63:
        return False, before
    return True, spec["record"](sel, *others) + (coeff, bit)


def seal_arm(emu, spec, before, sel, others, coeff, bit):
    """the setter's call of the shared core: its arguments where the context's record keeps them"""
    _, idx, row = spec["record"](sel, *others)
    stored = Rec5()
    got = emu.emu_seal_arm(INT_MAX if spec["max"] is None else spec["max"], Rec5(*before), sel, idx, row, coeff, bit, stored)
    return got, tuple(stored)


@pytest.mark.parametrize("name", list(SEALED))
def test_sealed_setters_accept_refuse_and_store_by_the_headers_rules(emu, name):
    spec = SEALED[name]
    sels = sorted({-2, -1, 0, 1} | ({INT_MAX} if spec["max"] is None else {spec["max"], spec["max"] + 1}))
    n = accepted = 0
    for before in (SEAL_DISARMED, SEAL_SENTINEL):
        for sel, others, coeff, bit in itertools.product(sels, itertools.product((-1, 0, 5), repeat=spec["others"]), (-1, 0, 7), (-1, 0, 63, 64)):
            got, stored = seal_arm(emu, spec, before, sel, others, coeff, bit)
            want_ok, want = seal_expected(spec, before, sel, others, coeff, bit)
            assert got == int(want_ok), (name, before, sel, others, coeff, bit)
            assert stored[0] == want[0], (name, before, sel, others, coeff, bit)
            if want[0] >= 0:                                        # (a disarmed hook's other fields mean nothing)
                assert stored == want, (name, before, sel, others, coeff, bit)
            if sel < 0:                                             # disarms, however bad the other arguments
                assert got == 1 and stored[0] == -1
            elif not want_ok and before == SEAL_SENTINEL:           # a refused call leaves the hook as it was
                assert stored == SEAL_SENTINEL
            n += 1
            accepted += got
    per_sel = 3 ** spec["others"] * 3 * 4
    assert n == 2 * len(sels) * per_sel
    # the two negative selectors accept every combination; each selector from 0 to the setter's highest accepts 2 values per other
    # index, 2 coefficients and 2 bits
    n_valid = sum(1 for v in sels if v >= 0 and (spec["max"] is None or v <= spec["max"]))
    assert n_valid == (3 if name != "galois_sealed" else 2)
    assert accepted == 2 * (2 * per_sel + n_valid * 2 ** spec["others"] * 2 * 2)


def test_sealed_setters_differ_where_the_header_says_so(emu):
    arm = lambda name, sel: seal_arm(emu, SEALED[name], SEAL_DISARMED, sel, (0,) * SEALED[name]["others"], 0, 0)[0]
    assert arm("tensor_sealed", 3) == 1 and arm("tensor_sealed", 4) == 0
    assert arm("galois_sealed", GAL_AT_INDEX) == 1 and arm("galois_sealed", GAL_AT_INDEX + 1) == 0
    for name in ("bsgs_sealed", "keyswitch_sealed", "ntt_sealed"):      # no upper bound at the setter
        assert arm(name, 4) == 1 and arm(name, INT_MAX) == 1


@pytest.mark.parametrize("name", list(SEALED))
def test_sealed_take_returns_the_armed_record_once(emu, name):
    spec = SEALED[name]
    others = (6, 2)[:spec["others"]]
    _, idx, row = spec["record"](1, *others)
    first, second, stored = Rec5(), Rec5(), Rec5()
    assert emu.emu_seal_take_twice(INT_MAX if spec["max"] is None else spec["max"], 1, idx, row, 1 << 40, 63, first, second, stored) == 1
    assert tuple(first) == spec["record"](1, *others) + (1 << 40, 63)
    assert second[0] == -1 and stored[0] == -1
    # a refused setter leaves nothing to take
    assert emu.emu_seal_take_twice(3, 1, idx, row, 0, 64, first, second, stored) == 0
    assert first[0] == -1 and second[0] == -1 and stored[0] == -1


@pytest.mark.parametrize("log_n", [1, 5, 16])
def test_sealed_hook_inside_the_call(emu, log_n):
    """row < rows and coeff < 2^log_n: the test every sealed call makes on the hook it took, before anything is launched"""
    N = 1 << log_n
    for row, coeff in itertools.product((0, 5), (0, N - 1)):
        assert emu.emu_seal_inside(row, coeff, 0, log_n) == 0               # a call of no rows has no word to hit
    for rows in (1, 6, 1 << 20):
        assert emu.emu_seal_inside(rows - 1, 0, rows, log_n) == 1
        assert emu.emu_seal_inside(rows, 0, rows, log_n) == 0
        assert emu.emu_seal_inside(rows - 1, N - 1, rows, log_n) == 1
        assert emu.emu_seal_inside(rows - 1, N, rows, log_n) == 0
        assert emu.emu_seal_inside(0, N - 1, rows, log_n) == 1 and emu.emu_seal_inside(0, N, rows, log_n) == 0
        assert emu.emu_seal_inside(rows, N, rows, log_n) == 0
