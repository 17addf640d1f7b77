"""The sealed forward transform's two C calls are declared, exported and bound, and refuse null arguments with a status -- no
compute calls: runs without a GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fhe_ntt_forward_sealed", "fhe_ntt_inverse_sealed_out")
INVALID = 1


def test_the_names_are_declared_exported_and_bound():
    from fhe_reliability_gpu_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fhe_mi355x.h")).read(), flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), f"{n} is not declared"
        assert hasattr(raw, n), f"{n} is not exported"
        assert n in _lib.EXPORTS and getattr(_lib.lib, n).argtypes is not None, f"{n} is not bound"
        # fhe_ntt_inverse_sealed's arguments with the output seal behind the input seal
        assert len(getattr(_lib.lib, n).argtypes) == len(_lib.lib.fhe_ntt_inverse_sealed.argtypes) + 1
    import fhe_reliability_gpu_amd as F
    assert callable(F.NttTables.ntt_sealed) and callable(F.NttTables.intt_sealed_out)
    doc = F.Engine.inject_fault_ntt_sealed.__doc__
    assert "ntt_sealed" in doc and "intt_sealed_out" in doc


def test_null_arguments_are_statuses():
    from fhe_reliability_gpu_amd._lib import lib
    for n in NAMES:
        assert getattr(lib, n)(None, None, None, None, None, 1, 1, 0, None, None, None, None) == INVALID
        assert b"null" in lib.fhe_last_error()
