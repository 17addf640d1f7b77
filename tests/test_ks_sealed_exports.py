"""The sealed key switch's five C calls are declared, exported and bound, refuse null arguments with a status, and the layout call
gives {0, dnum 2 M, dnum 2 M + the checked key switch's total, fused} on a host-filled plan (tests/emu/emu_ks_sealed_layout.cpp) --
no compute calls: runs without a GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
PKG = os.path.join(ROOT, "fhe_reliability_gpu_amd")
CSRC = os.path.join(PKG, "csrc")
NAMES = ("fhe_keyswitch_sealed_layout", "fhe_keyswitch_apply_sealed", "fhe_rotate_sealed_fused", "fhe_hmult_sealed_fused_key",
         "fhe_ctx_inject_fault_keyswitch_sealed")
INVALID = 1
CAP = 12
PATTERN = 0x5A5A5A5A


def test_the_five_names_are_declared_exported_and_bound():
    from fhe_reliability_gpu_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fhe_mi355x.h")).read(), flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), f"{n} is not declared"
        assert hasattr(raw, n), f"{n} is not exported"
        assert n in _lib.EXPORTS and getattr(_lib.lib, n).argtypes is not None, f"{n} is not bound"
    # the fused calls take exactly the sweep-based calls' arguments
    assert _lib.lib.fhe_rotate_sealed_fused.argtypes == _lib.lib.fhe_rotate_sealed.argtypes
    assert _lib.lib.fhe_hmult_sealed_fused_key.argtypes == _lib.lib.fhe_hmult_sealed.argtypes
    # fhe_keyswitch_apply_checked's, with the key's seal before the flags
    assert len(_lib.lib.fhe_keyswitch_apply_sealed.argtypes) == len(_lib.lib.fhe_keyswitch_apply_checked.argtypes) + 1
    import fhe_reliability_gpu_amd as F
    for m in ("apply_sealed", "apply_sealed_layout", "rotate_sealed_fused", "hmult_sealed_fused_key"):
        assert callable(getattr(F.KeySwitch, m))
    assert callable(F.Engine.inject_fault_keyswitch_sealed)


def test_null_arguments_are_statuses():
    from fhe_reliability_gpu_amd._lib import lib
    vp4, vp2 = (C.c_void_p * 4)(), (C.c_void_p * 2)()
    out = (C.c_int * 4)()
    for call in (lambda: lib.fhe_keyswitch_apply_sealed(None, None, None, None, None, None, None, None, None, None, None, None),
                 lambda: lib.fhe_rotate_sealed_fused(None, None, None, None, None, None, 3, None, None, vp2, None, vp2, None, None),
                 lambda: lib.fhe_hmult_sealed_fused_key(None, None, None, None, None, None, None, None, None, 1, None, vp4, None, vp2, None, None),
                 lambda: lib.fhe_ctx_inject_fault_keyswitch_sealed(None, 0, 0, 0),
                 lambda: lib.fhe_ctx_inject_fault_keyswitch_sealed(None, -1, 0, 0),
                 lambda: lib.fhe_keyswitch_sealed_layout(None, out)):
        assert call() == INVALID
        assert b"null" in lib.fhe_last_error()


@pytest.fixture(scope="module")
def layout():
    from fhe_reliability_gpu_amd import _lib      # the library the helper links against is loaded first
    so = os.path.join(EMU_DIR, "libemu_ks_sealed_layout.so")
    srcs = [os.path.join(EMU_DIR, "emu_ks_sealed_layout.cpp"), os.path.join(CSRC, "capi_internal.hpp"), os.path.join(CSRC, "fault_hook.hpp"), _lib.LIB_PATH]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call([hipcc, "-O1", "-std=c++17", "--cuda-host-only", "-x", "hip", "-shared", "-fPIC", "-I" + CSRC, srcs[0], "-L" + PKG,
                               "-lfhe_mi355x", "-Wl,-rpath," + PKG, "-o", so])
    L = C.CDLL(so)
    L.emu_ks_sealed_layout.restype = C.c_int
    L.emu_ks_sealed_layout.argtypes = [C.c_int] * 4 + [C.c_ulonglong, C.POINTER(C.c_int)]

    def get(logn, Lq, K, dnum, plain=0):
        """(status, the four words); the words behind the array keep their pattern"""
        out = (C.c_int * 6)(*[PATTERN] * 6)
        rc = L.emu_ks_sealed_layout(logn, Lq, K, dnum, plain, out)
        assert list(out)[4:] == [PATTERN] * 2
        return rc, list(out)[:4]
    return get


def checked_total(L, K, d, bgv):
    """the checked key switch's block: intt_in [L], extend [d][M], ntt_ext [d][M], mac [2][M], intt_special [2][K], moddown [2][K + L],
    ntt_conv [2][L], tail [2][L]; BGV then scale_special [2][K], scale_conv [2][L]"""
    M = L + K
    return L + 2 * d * M + 2 * M + 2 * K + 2 * (K + L) + 4 * L + (2 * K + 2 * L if bgv else 0)


@pytest.mark.parametrize("plain", [0, 65537])
def test_layout_is_the_key_rows_then_the_checked_block(layout, plain):
    for logn, L, K, dnum in ((10, 4, 2, 2), (13, 3, 1, 3), (14, 6, 2, 3), (17, 32, 8, 4), (16, 44, 4, 11), (10, 13, 1, 13), (10, 5, 1, 1)):
        rc, out = layout(logn, L, K, dnum, plain)
        rows = dnum * 2 * (L + K)
        assert rc == 0 and out == [0, rows, rows + checked_total(L, K, dnum, bool(plain)), 1 if dnum <= CAP else 0], (logn, L, K, dnum)


def test_fused_is_one_up_to_the_cap_and_zero_above(layout):
    for dnum in range(1, 17):
        rc, out = layout(10, 16, 1, dnum)
        assert rc == 0 and out[3] == (1 if dnum <= CAP else 0), dnum
    # BASELINE configs 4 and 5 (dnum = 4) are on the fused route, and so is a plan of 11 digits
    assert layout(17, 32, 8, 4)[1][3] == 1 and layout(16, 44, 11, 4)[1][3] == 1 and layout(16, 44, 4, 11)[1][3] == 1
