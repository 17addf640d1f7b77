"""The sealed negacyclic product's two C calls are declared, exported and bound, the Python names exist, and null arguments come back
as a status -- no compute calls: runs without a GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fhe_polymul_sealed", "fhe_ctx_inject_fault_polymul_sealed")
INVALID = 1


def test_the_names_are_declared_exported_and_bound():
    from fhe_reliability_gpu_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fhe_mi355x.h")).read(), flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), f"{n} is not declared"
        assert hasattr(raw, n), f"{n} is not exported"
        assert n in _lib.EXPORTS and getattr(_lib.lib, n).argtypes is not None, f"{n} is not bound"
    # fhe_polymul_checked's arguments with the three seals in front of the flags
    assert len(_lib.lib.fhe_polymul_sealed.argtypes) == len(_lib.lib.fhe_polymul_checked.argtypes) + 3
    import fhe_reliability_gpu_amd as F
    assert callable(F.Abft.polymul_sealed) and callable(F.Engine.inject_fault_polymul_sealed)
    assert "polymul_sealed" in F.Engine.inject_fault_polymul_sealed.__doc__


def test_null_arguments_are_statuses():
    from fhe_reliability_gpu_amd._lib import lib
    assert lib.fhe_polymul_sealed(None, None, None, None, None, None, 1, 1, 0, None, None, None, None, None) == INVALID
    assert b"null" in lib.fhe_last_error()
    assert lib.fhe_ctx_inject_fault_polymul_sealed(None, 0, 0, 0, 0) == INVALID
    assert b"null" in lib.fhe_last_error()
