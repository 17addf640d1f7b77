"""The one-shot test hooks of the checked calls on the CPU (tests/emu/emu_fault_hook.cpp compiles fault_hook.hpp, the records
the context stores and the code every fhe_ctx_inject_fault_* setter and every checked call shares): what the setters accept,
refuse and store equals a table written here from the rules of include/fhe_mi355x.h, take() hands a hook out once, and the
check-record builder arms exactly the launch whose flags hold the fault's unit -- without a GPU."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "fhe_reliability_gpu_amd", "csrc")
Rec6, Rec4 = C.c_longlong * 6, C.c_longlong * 4

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
    so = os.path.join(EMU_DIR, "libemu_fault_hook.so")
    srcs = [os.path.join(EMU_DIR, "emu_fault_hook.cpp")] + [os.path.join(CSRC, f) for f in ("fault_hook.hpp", "galois_check.hpp", "modarith.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, srcs[0], "-o", so])
    L = C.CDLL(so)
    ll, i = C.c_longlong, C.c_int
    L.emu_hook_stages.argtypes = [i]
    L.emu_hook_arm.argtypes = [i, Rec6, i, i, i, i, ll, i, Rec6]
    L.emu_hook_take_twice.argtypes = [i, i, i, i, i, ll, i, Rec6, Rec6, Rec6]
    L.emu_point_arm.argtypes = [i, Rec4, i, i, ll, i, Rec4]
    L.emu_point_take_twice.argtypes = [i, i, i, ll, i, Rec4, Rec4, Rec4]
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
