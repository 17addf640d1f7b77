"""The sealed rescale's and the sealed tail's five C calls are declared, exported and bound, refuse null arguments with a status, the
layout call gives its numbers on host-filled plans, and a null input seal is refused before any device work while taking an armed
hook with it (tests/emu/emu_rescale_sealed_layout.cpp) -- no compute calls: runs without a GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
PKG = os.path.join(ROOT, "fhe_reliability_gpu_amd")
CSRC = os.path.join(PKG, "csrc")
NAMES = ("fhe_ctx_inject_fault_subscale_sealed", "fhe_rescale_sealed_layout", "fhe_rescale_sealed", "fhe_hmult_sealed_out", "fhe_rotate_sealed_out")
INVALID = 1
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
    # the siblings' arguments; fhe_rescale_checked's with the input's and the output's seal before the flags
    assert _lib.lib.fhe_hmult_sealed_out.argtypes == _lib.lib.fhe_hmult_sealed_fused_key.argtypes
    assert _lib.lib.fhe_rotate_sealed_out.argtypes == _lib.lib.fhe_rotate_sealed_in.argtypes
    assert len(_lib.lib.fhe_rescale_sealed.argtypes) == len(_lib.lib.fhe_rescale_checked.argtypes) + 2
    import fhe_reliability_gpu_amd as F
    for m in ("rescale_sealed", "rescale_sealed_layout", "hmult_sealed_out", "rotate_sealed_out"):
        assert callable(getattr(F.KeySwitch, m))
    assert callable(F.Engine.inject_fault_subscale_sealed)


def test_null_arguments_are_statuses():
    from fhe_reliability_gpu_amd._lib import lib
    vp2 = (C.c_void_p * 2)()
    out = (C.c_int * 8)()
    for call in (lambda: lib.fhe_rescale_sealed(None, None, None, None, 2, None, None, None, None, None),
                 lambda: lib.fhe_hmult_sealed_out(None, None, None, None, None, None, None, None, None, 1, None, vp2, None, vp2, None, None),
                 lambda: lib.fhe_rotate_sealed_out(None, None, None, None, None, None, 3, None, None, vp2, None, vp2, None, None),
                 lambda: lib.fhe_ctx_inject_fault_subscale_sealed(None, 0, 0, 0, 0),
                 lambda: lib.fhe_ctx_inject_fault_subscale_sealed(None, -1, 0, 0, 0),
                 lambda: lib.fhe_rescale_sealed_layout(None, 2, out)):
        assert call() == INVALID
        assert b"null" in lib.fhe_last_error()


@pytest.fixture(scope="module")
def helper():
    from fhe_reliability_gpu_amd import _lib      # the library the helper links against is loaded first
    so = os.path.join(EMU_DIR, "libemu_rescale_sealed_layout.so")
    srcs = [os.path.join(EMU_DIR, "emu_rescale_sealed_layout.cpp"), os.path.join(CSRC, "capi_internal.hpp"), os.path.join(CSRC, "fault_hook.hpp"), _lib.LIB_PATH]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call([hipcc, "-O1", "-std=c++17", "--cuda-host-only", "-x", "hip", "-shared", "-fPIC", "-I" + CSRC, srcs[0], "-L" + PKG,
                               "-lfhe_mi355x", "-Wl,-rpath," + PKG, "-o", so])
    L = C.CDLL(so)
    L.emu_rescale_sealed_layout.restype = C.c_int
    L.emu_rescale_sealed_layout.argtypes = [C.c_int] * 4 + [C.c_ulonglong, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.emu_null_seal_in.restype = C.c_int
    L.emu_null_seal_in.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int)]
    return L


def checked_total(L, n, bgv):
    """the checked rescale's block: intt_last [n], reduce [n][R], ntt_delta [n][R], scale [n][R]; BGV then scale_last [n], scale_delta [n][R]"""
    R = L - 1
    return n + 3 * n * R + (n + n * R if bgv else 0)


@pytest.mark.parametrize("plain", [0, 65537])
def test_layout_is_input_rows_then_the_checked_rescales_block(helper, plain):
    for logn, L, K, dnum in PLANS:
        for n in (1, 2, 3):
            out = (C.c_int * 6)(*[PATTERN] * 6)
            inner = (C.c_int * 10)(*[PATTERN] * 10)
            assert helper.emu_rescale_sealed_layout(logn, L, K, dnum, plain, n, out, inner) == 0
            stages = 6 if plain else 4
            assert inner[stages] == checked_total(L, n, bool(plain))
            assert list(out) == [0, n * L, n * L + inner[stages], 0, PATTERN, PATTERN], (logn, L, K, dnum, n)
    # a ciphertext has 1 to 3 parts, and a prime must be left to drop
    from fhe_reliability_gpu_amd._lib import lib
    out = (C.c_int * 6)(*[PATTERN] * 6)
    inner = (C.c_int * 10)()
    for shape, n in (((10, 4, 2, 2), 0), ((10, 4, 2, 2), 4), ((10, 1, 1, 1), 2)):
        assert helper.emu_rescale_sealed_layout(*shape, plain, n, out, inner) == INVALID, (shape, n)
    assert list(out) == [PATTERN] * 6


def test_a_null_input_seal_is_refused_before_device_work_and_takes_the_hook(helper):
    from fhe_reliability_gpu_amd._lib import lib
    out = (C.c_int * 4)()
    assert helper.emu_null_seal_in(10, 4, 2, 2, out) == 0
    status, point_before, point_after, flags_untouched = list(out)
    assert status == INVALID and b"null" in lib.fhe_last_error()
    assert point_before == 1 and point_after == -1
    assert flags_untouched == 1
