"""The repair calls are declared in include/fhe_mi355x.h, exported by the library and bound by the ctypes layer, null arguments are
statuses, and the flag layouts of the repairing composites are the sealed composites' plus one report block -- without a GPU.
tests/emu/emu_seal_repair_layout.cpp hands the layout calls a plan structure filled on the host."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
PKG = os.path.join(ROOT, "fhe_reliability_gpu_amd")
CSRC = os.path.join(PKG, "csrc")
NAMES = ("fhe_seal_locator", "fhe_seal_repair", "fhe_hmult_sealed_repair_layout", "fhe_hmult_sealed_repair", "fhe_rotate_sealed_repair_layout",
         "fhe_rotate_sealed_repair")
INVALID = 1


def test_every_repair_call_is_declared_exported_and_bound():
    from fhe_reliability_gpu_amd import _lib
    header = open(os.path.join(ROOT, "include", "fhe_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(fhe_[a-z0-9_]+)\s*\(", text))
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n in declared, f"{n} not declared in fhe_mi355x.h"
        assert hasattr(raw, n), f"{n} not exported by the library"
        assert n in _lib.EXPORTS and getattr(_lib.lib, n).argtypes is not None, f"{n} not bound"
    assert len(_lib.lib.fhe_seal_locator.argtypes) == 8 and len(_lib.lib.fhe_seal_repair.argtypes) == 11
    # the sealed composites' arguments plus the locators in, the key's locator and the locators out
    assert len(_lib.lib.fhe_hmult_sealed_repair.argtypes) == len(_lib.lib.fhe_hmult_sealed.argtypes) + 3 == 19
    assert len(_lib.lib.fhe_rotate_sealed_repair.argtypes) == len(_lib.lib.fhe_rotate_sealed.argtypes) + 3 == 17
    # the outcomes are public constants of the header and of the package, with the same values
    import fhe_reliability_gpu_amd as F
    for name, value in (("CLEAN", 0), ("REPAIRED", 1), ("UNCORRECTABLE", 2), ("TRANSIENT", 3), ("SUSPECT", 4)):
        assert re.search(rf"#define\s+FHE_SEAL_{name}\s+{value}\b", header), name
        assert getattr(F, "SEAL_" + name) == value


def test_the_python_layer_exposes_the_repair_calls():
    import fhe_reliability_gpu_amd as F
    for cls, names in ((F.NttTables, ("seal_locator", "seal_repair")),
                       (F.KeySwitch, ("seal_key_locator", "hmult_sealed_repair", "rotate_sealed_repair", "hmult_sealed_repair_layout",
                                      "rotate_sealed_repair_layout"))):
        for n in names:
            assert callable(getattr(cls, n)), n


def test_null_arguments_are_statuses():
    from fhe_reliability_gpu_amd._lib import lib
    out = (C.c_int * 10)()
    assert lib.fhe_hmult_sealed_repair_layout(None, 1, out) == INVALID and lib.fhe_rotate_sealed_repair_layout(None, out) == INVALID
    assert lib.fhe_seal_locator(None, None, None, None, 1, 1, 0, None) == INVALID
    assert lib.fhe_seal_repair(None, None, None, None, None, 1, 1, 0, None, None, None) == INVALID
    assert lib.fhe_hmult_sealed_repair(*([None] * 9), 1, *([None] * 9)) == INVALID
    assert lib.fhe_rotate_sealed_repair(*([None] * 6), 5, *([None] * 10)) == INVALID


@pytest.fixture(scope="module")
def layouts():
    from fhe_reliability_gpu_amd import _lib      # the library the helper links against is loaded first
    so = os.path.join(EMU_DIR, "libemu_seal_repair_layout.so")
    srcs = [os.path.join(EMU_DIR, "emu_seal_repair_layout.cpp"), os.path.join(CSRC, "capi_internal.hpp"), os.path.join(CSRC, "fault_hook.hpp"), _lib.LIB_PATH]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call([hipcc, "-O1", "-std=c++17", "--cuda-host-only", "-x", "hip", "-shared", "-fPIC", "-I" + CSRC, srcs[0], "-L" + PKG,
                               "-lfhe_mi355x", "-Wl,-rpath," + PKG, "-o", so])
    L = C.CDLL(so)
    L.emu_repair_layouts.restype = C.c_int
    L.emu_repair_layouts.argtypes = [C.c_int] * 4 + [C.c_ulonglong, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]

    def get(log_n, L_, K, dnum, plain, rescale):
        sealed, repair = (C.c_int * 14)(), (C.c_int * 18)()
        assert L.emu_repair_layouts(log_n, L_, K, dnum, plain, rescale, sealed, repair) == 0
        return list(sealed), list(repair)
    return get


@pytest.mark.parametrize("plain", [0, 65537])
@pytest.mark.parametrize("shape", [(10, 4, 2, 2), (13, 3, 1, 3), (14, 6, 2, 3), (17, 32, 8, 4)])
def test_repair_layouts_are_the_sealed_layouts_plus_the_report_block(layouts, shape, plain):
    log_n, L, K, dnum = shape
    key = dnum * 2 * (L + K)
    for rescale in (0, 1):
        sealed, repair = layouts(log_n, L, K, dnum, plain, rescale)
        hm, rot = repair[:10], repair[10:]
        # the sealed call's layout, word for word, its total included
        assert hm[:7] == sealed[:7] and rot[:5] == sealed[8:13]
        # then the report block: 16-byte aligned, four uint64 = eight flag words per input and key row
        rows = 4 * L + key
        assert hm[7] % 4 == 0 and 0 <= hm[7] - hm[6] < 4 and hm[8] == hm[7] + 8 * rows and hm[9] == 0 and hm[5] == rows
        rows = 2 * L + key
        assert rot[5] % 4 == 0 and 0 <= rot[5] - rot[4] < 4 and rot[6] == rot[5] + 8 * rows and rot[7] == 0 and rot[3] == rows
