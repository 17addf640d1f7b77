"""The sealed inverse transform's six C calls are declared, exported and bound, refuse null arguments with a status, the two
layout calls give their numbers on host-filled plans, and a null input seal is refused before any device work while taking an
armed hook with it (tests/emu/emu_ntt_sealed_layout.cpp) -- no compute calls: runs without a GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
PKG = os.path.join(ROOT, "fhe_reliability_gpu_amd")
CSRC = os.path.join(PKG, "csrc")
NAMES = ("fhe_ntt_inverse_sealed", "fhe_ctx_inject_fault_ntt_sealed", "fhe_keyswitch_sealed_in_layout", "fhe_keyswitch_apply_sealed_in",
         "fhe_rotate_sealed_in_layout", "fhe_rotate_sealed_in")
INVALID = 1
CAP = 12
PATTERN = 0x5A5A5A5A
PLANS = ((10, 4, 2, 2), (13, 3, 1, 3), (14, 6, 2, 3), (17, 32, 8, 4), (10, 13, 1, 13))


def test_the_names_are_declared_exported_and_bound():
    from fhe_reliability_gpu_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fhe_mi355x.h")).read(), flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), f"{n} is not declared"
        assert hasattr(raw, n), f"{n} is not exported"
        assert n in _lib.EXPORTS and getattr(_lib.lib, n).argtypes is not None, f"{n} is not bound"
    # fhe_rotate_sealed_fused's arguments; fhe_keyswitch_apply_sealed's with the input's seal before the key's
    assert _lib.lib.fhe_rotate_sealed_in.argtypes == _lib.lib.fhe_rotate_sealed_fused.argtypes
    assert len(_lib.lib.fhe_keyswitch_apply_sealed_in.argtypes) == len(_lib.lib.fhe_keyswitch_apply_sealed.argtypes) + 1
    # fhe_ntt_inverse_checked's with a destination and a seal
    assert len(_lib.lib.fhe_ntt_inverse_sealed.argtypes) == len(_lib.lib.fhe_ntt_inverse_checked.argtypes) + 2
    import fhe_reliability_gpu_amd as F
    for m in ("apply_sealed_in", "apply_sealed_in_layout", "rotate_sealed_in", "rotate_sealed_in_layout"):
        assert callable(getattr(F.KeySwitch, m))
    assert callable(F.NttTables.intt_sealed)
    assert callable(F.Engine.inject_fault_ntt_sealed)


def test_null_arguments_are_statuses():
    from fhe_reliability_gpu_amd._lib import lib
    vp2 = (C.c_void_p * 2)()
    out = (C.c_int * 8)()
    for call in (lambda: lib.fhe_ntt_inverse_sealed(None, None, None, None, None, 1, 1, 0, None, None, None),
                 lambda: lib.fhe_keyswitch_apply_sealed_in(None, None, None, None, None, None, None, None, None, None, None, None, None),
                 lambda: lib.fhe_rotate_sealed_in(None, None, None, None, None, None, 3, None, None, vp2, None, vp2, None, None),
                 lambda: lib.fhe_ctx_inject_fault_ntt_sealed(None, 0, 0, 0),
                 lambda: lib.fhe_ctx_inject_fault_ntt_sealed(None, -1, 0, 0),
                 lambda: lib.fhe_keyswitch_sealed_in_layout(None, out),
                 lambda: lib.fhe_rotate_sealed_in_layout(None, out)):
        assert call() == INVALID
        assert b"null" in lib.fhe_last_error()


@pytest.fixture(scope="module")
def helper():
    from fhe_reliability_gpu_amd import _lib      # the library the helper links against is loaded first
    so = os.path.join(EMU_DIR, "libemu_ntt_sealed_layout.so")
    srcs = [os.path.join(EMU_DIR, "emu_ntt_sealed_layout.cpp"), os.path.join(CSRC, "capi_internal.hpp"), os.path.join(CSRC, "fault_hook.hpp"), _lib.LIB_PATH]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call([hipcc, "-O1", "-std=c++17", "--cuda-host-only", "-x", "hip", "-shared", "-fPIC", "-I" + CSRC, srcs[0], "-L" + PKG,
                               "-lfhe_mi355x", "-Wl,-rpath," + PKG, "-o", so])
    L = C.CDLL(so)
    L.emu_ntt_sealed_layout.restype = C.c_int
    L.emu_ntt_sealed_layout.argtypes = [C.c_int] * 5 + [C.c_ulonglong, C.POINTER(C.c_int)]
    L.emu_null_seal_c.restype = C.c_int
    L.emu_null_seal_c.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int)]
    return L


def layout(helper, which, n, logn, Lq, K, dnum, plain=0):
    """(status, the n words); the words behind the array keep their pattern"""
    out = (C.c_int * (n + 2))(*[PATTERN] * (n + 2))
    rc = helper.emu_ntt_sealed_layout(which, logn, Lq, K, dnum, plain, out)
    assert list(out)[n:] == [PATTERN] * 2
    return rc, list(out)[:n]


def checked_total(L, K, d, bgv):
    """the checked key switch's block: intt_in [L], extend [d][M], ntt_ext [d][M], mac [2][M], intt_special [2][K], moddown [2][K + L],
    ntt_conv [2][L], tail [2][L]; BGV then scale_special [2][K], scale_conv [2][L]"""
    M = L + K
    return L + 2 * d * M + 2 * M + 2 * K + 2 * (K + L) + 4 * L + (2 * K + 2 * L if bgv else 0)


@pytest.mark.parametrize("plain", [0, 65537])
def test_keyswitch_layout_is_c_rows_key_rows_checked_block(helper, plain):
    for logn, L, K, dnum in PLANS:
        rc, out = layout(helper, 0, 5, logn, L, K, dnum, plain)
        rows = dnum * 2 * (L + K)
        assert rc == 0 and out == [0, L, L + rows, L + rows + checked_total(L, K, dnum, bool(plain)), 1 if dnum <= CAP else 0], (logn, L, K, dnum)


@pytest.mark.parametrize("plain", [0, 65537])
def test_rotate_layout_is_c0_c1_sigma_key_checked_block(helper, plain):
    for logn, L, K, dnum in PLANS:
        rc, out = layout(helper, 1, 7, logn, L, K, dnum, plain)
        rows = dnum * 2 * (L + K)
        assert rc == 0 and out == [0, L, 2 * L, 3 * L, 3 * L + rows, 3 * L + rows + checked_total(L, K, dnum, bool(plain)), 1 if dnum <= CAP else 0], (logn, L, K, dnum)


def test_a_null_input_seal_is_refused_before_device_work_and_takes_the_hook(helper):
    from fhe_reliability_gpu_amd._lib import lib
    out = (C.c_int * 4)()
    assert helper.emu_null_seal_c(10, 4, 2, 2, out) == 0
    status, row_before, row_after, flags_untouched = list(out)
    assert status == INVALID and b"null" in lib.fhe_last_error()
    assert row_before == 1 and row_after == -1
    assert flags_untouched == 1
