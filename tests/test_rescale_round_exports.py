"""The two entry points of the rescale's rounding mode are exported, bound in _lib.EXPORTS and declared in the header; what they
refuse on the host alone needs no GPU."""
import ctypes as C
import os

from fhe_reliability_gpu_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fhe_keyswitch_set_rescale_rounding", "fhe_keyswitch_get_rescale_rounding")
FHE_ERR_INVALID = 1


def test_symbols_are_exported_bound_and_declared():
    header = open(os.path.join(ROOT, "include", "fhe_mi355x.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS
        fn = getattr(_lib.lib, name)
        assert fn.restype is C.c_int
        assert f"int {name}(" in header
    assert _lib.lib.fhe_keyswitch_set_rescale_rounding.argtypes == [C.c_void_p, C.c_int]
    assert _lib.lib.fhe_keyswitch_get_rescale_rounding.argtypes == [C.c_void_p, C.POINTER(C.c_int)]


def test_host_only_refusals():
    lib = _lib.lib
    # the mode is judged before the plan: a mode other than 0 or 1 is refused as such
    for mode in (2, -1, 7):
        assert lib.fhe_keyswitch_set_rescale_rounding(None, mode) == FHE_ERR_INVALID
        assert b"0 (floor) or 1 (nearest)" in lib.fhe_last_error()
    for mode in (0, 1):
        assert lib.fhe_keyswitch_set_rescale_rounding(None, mode) == FHE_ERR_INVALID
        assert b"null" in lib.fhe_last_error()
    mode = C.c_int(5)
    assert lib.fhe_keyswitch_get_rescale_rounding(None, C.byref(mode)) == FHE_ERR_INVALID
    assert mode.value == 5
