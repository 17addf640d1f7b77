"""The sealed tensor product's four C calls are declared, exported and bound, refuse null arguments with a status, and the layout
call gives {0, R, 2R, 3R, 4R, 7R} -- no compute calls: runs without a GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fhe_tensor_product_sealed_layout", "fhe_tensor_product_sealed", "fhe_ctx_inject_fault_tensor_sealed", "fhe_hmult_sealed_fused")
INVALID = 1


def test_the_four_names_are_declared_exported_and_bound():
    from fhe_reliability_gpu_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fhe_mi355x.h")).read(), flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), f"{n} is not declared"
        assert hasattr(raw, n), f"{n} is not exported"
        assert n in _lib.EXPORTS and getattr(_lib.lib, n).argtypes is not None, f"{n} is not bound"
    # the fused multiply takes exactly the sealed multiply's arguments
    assert _lib.lib.fhe_hmult_sealed_fused.argtypes == _lib.lib.fhe_hmult_sealed.argtypes
    import fhe_reliability_gpu_amd as F
    for m in ("tensor_sealed", "tensor_sealed_layout", "hmult_sealed_fused"):
        assert callable(getattr(F.KeySwitch, m))
    assert callable(F.Engine.inject_fault_tensor_sealed)


def test_null_arguments_are_statuses():
    from fhe_reliability_gpu_amd._lib import lib
    assert lib.fhe_last_error is not None
    vp4, vp3 = (C.c_void_p * 4)(), (C.c_void_p * 3)()
    assert lib.fhe_tensor_product_sealed(None, None, None, None, None, None, None, None, None, 1, 1, 0, vp4, vp3, None, None) == INVALID
    assert b"null" in lib.fhe_last_error()
    assert lib.fhe_hmult_sealed_fused(None, None, None, None, None, None, None, None, None, 1, None, vp4, None, None, None, None) == INVALID
    assert lib.fhe_ctx_inject_fault_tensor_sealed(None, 0, 0, 0, 0) == INVALID
    assert lib.fhe_ctx_inject_fault_tensor_sealed(None, -1, 0, 0, 0) == INVALID
    assert lib.fhe_tensor_product_sealed_layout(1, 1, None) == INVALID


def test_layout_is_four_operand_blocks_then_the_tensor_block():
    from fhe_reliability_gpu_amd._lib import lib
    for n_poly, limbs in ((1, 1), (1, 6), (3, 4), (2, 44), (3 * 8192 + 1, 1), (0, 5)):
        out = (C.c_int * 6)(*([-1] * 6))
        assert lib.fhe_tensor_product_sealed_layout(n_poly, limbs, out) == 0
        R = n_poly * limbs
        assert list(out) == [0, R, 2 * R, 3 * R, 4 * R, 7 * R]
    out = (C.c_int * 6)()
    assert lib.fhe_tensor_product_sealed_layout((1 << 24) + 1, 1, out) == INVALID
