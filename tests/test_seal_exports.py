"""The seal calls are declared in include/fhe_mi355x.h, exported by the library and bound by the ctypes layer, and the flag layouts
of the two sealed composites are the sum of their parts -- without a GPU.  The layout calls read a plan's shape and nothing on the
device, so tests/emu/emu_seal_layout.cpp hands them a plan structure filled on the host."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
PKG = os.path.join(ROOT, "fhe_reliability_gpu_amd")
CSRC = os.path.join(PKG, "csrc")
NAMES = ("fhe_seal", "fhe_seal_verify", "fhe_ctx_inject_fault_seal", "fhe_hmult_sealed_layout", "fhe_hmult_sealed", "fhe_rotate_sealed_layout",
         "fhe_rotate_sealed")
INVALID = 1


def test_every_seal_call_is_declared_exported_and_bound():
    from fhe_reliability_gpu_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fhe_mi355x.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fhe_[a-z0-9_]+)\s*\(", text))
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n in declared, f"{n} not declared in fhe_mi355x.h"
        assert hasattr(raw, n), f"{n} not exported by the library"
        assert n in _lib.EXPORTS and getattr(_lib.lib, n).argtypes is not None, f"{n} not bound"
    # the pointer-array arguments of the composites: seals in, key seal, seals out, flags, stream
    assert len(_lib.lib.fhe_hmult_sealed.argtypes) == 16 and len(_lib.lib.fhe_rotate_sealed.argtypes) == 14
    assert len(_lib.lib.fhe_seal.argtypes) == 8 and len(_lib.lib.fhe_seal_verify.argtypes) == 9


def test_the_python_layer_exposes_the_seal_calls():
    import fhe_reliability_gpu_amd as F
    for cls, names in ((F.NttTables, ("seal", "seal_verify")),
                       (F.KeySwitch, ("seal_key", "hmult_sealed", "rotate_sealed", "hmult_sealed_layout", "rotate_sealed_layout"))):
        for n in names:
            assert callable(getattr(cls, n)), n
    assert F.SEAL_P == 2**61 - 1 and (F.SEAL_SUM, F.SEAL_RANGE) == (1, 2)


def test_null_arguments_are_statuses():
    from fhe_reliability_gpu_amd._lib import lib
    out = (C.c_int * 8)()
    assert lib.fhe_hmult_sealed_layout(None, 1, out) == INVALID and lib.fhe_rotate_sealed_layout(None, out) == INVALID
    assert lib.fhe_ctx_inject_fault_seal(None, 0, 0, 0) == INVALID
    assert lib.fhe_seal(None, None, None, None, 1, 1, 0, None) == INVALID
    assert lib.fhe_seal_verify(None, None, None, None, 1, 1, 0, None, None) == INVALID


@pytest.fixture(scope="module")
def layouts():
    from fhe_reliability_gpu_amd import _lib      # the library the helper links against is loaded first
    so = os.path.join(EMU_DIR, "libemu_seal_layout.so")
    srcs = [os.path.join(EMU_DIR, "emu_seal_layout.cpp"), os.path.join(CSRC, "capi_internal.hpp"), os.path.join(CSRC, "fault_hook.hpp"), _lib.LIB_PATH]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call([hipcc, "-O1", "-std=c++17", "--cuda-host-only", "-x", "hip", "-shared", "-fPIC", "-I" + CSRC, srcs[0], "-L" + PKG,
                               "-lfhe_mi355x", "-Wl,-rpath," + PKG, "-o", so])
    L = C.CDLL(so)
    L.emu_sealed_layouts.restype = C.c_int
    L.emu_sealed_layouts.argtypes = [C.c_int] * 4 + [C.c_ulonglong, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]

    def get(log_n, L_, K, dnum, plain, rescale):
        sealed, inner = (C.c_int * 14)(), (C.c_int * 5)()
        assert L.emu_sealed_layouts(log_n, L_, K, dnum, plain, rescale, sealed, inner) == 0
        return list(sealed), list(inner)
    return get


@pytest.mark.parametrize("plain", [0, 65537])
@pytest.mark.parametrize("shape", [(10, 4, 2, 2), (13, 3, 1, 3), (14, 6, 2, 3), (17, 32, 8, 4)])
def test_sealed_layouts_are_the_sum_of_their_parts(layouts, shape, plain):
    log_n, L, K, dnum = shape
    key = dnum * 2 * (L + K)
    for rescale in (0, 1):
        sealed, inner = layouts(log_n, L, K, dnum, plain, rescale)
        hm, rot = sealed[:8], sealed[8:]
        # [a0][a1][b0][b1], L rows each, then the key's rows, then the checked multiply's own block
        assert hm[:5] == [0, L, 2 * L, 3 * L, 4 * L]
        assert hm[5] == 4 * L + key and hm[6] == hm[5] + inner[3] and hm[7] == 0
        # [c0][c1][key][the checked key switch's block]
        assert rot == [0, L, 2 * L, 2 * L + key, 2 * L + key + inner[4], 0]
    # the embedded blocks are the existing layouts': the multiply's grows by the rescale block only
    (_, with_r), (_, without) = layouts(log_n, L, K, dnum, plain, 1), layouts(log_n, L, K, dnum, plain, 0)
    assert with_r[:3] == without[:3] and with_r[3] > without[3] == without[2] and with_r[4] == without[4]
