"""The sealed Galois permutation's four C calls are declared, exported and bound, refuse null arguments with a status, and the
layout call gives {0, L, L + dnum 2 M, L + n_rot (L + dnum 2 M), that + the checked hoisted rotations' total, fused} on a host-filled
plan (tests/emu/emu_hoisted_sealed_layout.cpp) -- no compute calls: runs without a GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
PKG = os.path.join(ROOT, "fhe_reliability_gpu_amd")
CSRC = os.path.join(PKG, "csrc")
NAMES = ("fhe_automorphism_ntt_sealed", "fhe_rotate_hoisted_sealed_layout", "fhe_rotate_hoisted_sealed", "fhe_ctx_inject_fault_galois_sealed")
INVALID, UNSUPPORTED = 1, 3
CAP = 12
PATTERN = 0x5A5A5A5A
PLANS = ((10, 4, 2, 2), (13, 3, 1, 3), (14, 6, 2, 3), (17, 32, 8, 4), (10, 13, 1, 13))


def test_the_four_names_are_declared_exported_and_bound():
    from fhe_reliability_gpu_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fhe_mi355x.h")).read(), flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), f"{n} is not declared"
        assert hasattr(raw, n), f"{n} is not exported"
        assert n in _lib.EXPORTS and getattr(_lib.lib, n).argtypes is not None, f"{n} is not bound"
    # fhe_rotate_hoisted_checked's arguments, with the four seal arrays before the flags
    checked = _lib.lib.fhe_rotate_hoisted_checked.argtypes
    sealed = _lib.lib.fhe_rotate_hoisted_sealed.argtypes
    assert len(sealed) == len(checked) + 4 and list(sealed[:len(checked) - 2]) == list(checked[:-2]) and list(sealed[-2:]) == list(checked[-2:])
    assert _lib.lib.fhe_rotate_hoisted_sealed_layout.argtypes == _lib.lib.fhe_rotate_hoisted_checked_layout.argtypes
    import fhe_reliability_gpu_amd as F
    assert callable(F.automorphism_sealed)
    for m in ("rotate_hoisted_sealed", "rotate_hoisted_sealed_layout"):
        assert callable(getattr(F.KeySwitch, m))
    assert callable(F.Engine.inject_fault_galois_sealed)


def test_null_arguments_are_statuses():
    from fhe_reliability_gpu_amd._lib import lib
    vp2 = (C.c_void_p * 2)()
    out = (C.c_int * 6)()
    for call in (lambda: lib.fhe_automorphism_ntt_sealed(None, None, None, None, None, None, 1, 1, 0, 3, None, None),
                 lambda: lib.fhe_rotate_hoisted_sealed(None, None, None, None, None, None, None, None, 1, None, vp2, None, None, None, None, None),
                 lambda: lib.fhe_ctx_inject_fault_galois_sealed(None, 0, 0, 0, 0, 0),
                 lambda: lib.fhe_ctx_inject_fault_galois_sealed(None, 0, -1, 0, 0, 0),
                 lambda: lib.fhe_rotate_hoisted_sealed_layout(None, 1, out)):
        assert call() == INVALID
        assert b"null" in lib.fhe_last_error()


@pytest.fixture(scope="module")
def layout():
    from fhe_reliability_gpu_amd import _lib      # the library the helper links against is loaded first
    so = os.path.join(EMU_DIR, "libemu_hoisted_sealed_layout.so")
    srcs = [os.path.join(EMU_DIR, "emu_hoisted_sealed_layout.cpp"), os.path.join(CSRC, "capi_internal.hpp"), os.path.join(CSRC, "fault_hook.hpp"), _lib.LIB_PATH]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call([hipcc, "-O1", "-std=c++17", "--cuda-host-only", "-x", "hip", "-shared", "-fPIC", "-I" + CSRC, srcs[0], "-L" + PKG,
                               "-lfhe_mi355x", "-Wl,-rpath," + PKG, "-o", so])
    L = C.CDLL(so)
    L.emu_hoisted_sealed_layout.restype = C.c_int
    L.emu_hoisted_sealed_layout.argtypes = [C.c_int] * 4 + [C.c_ulonglong, C.c_ulonglong, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]

    def get(logn, Lq, K, dnum, n_rot, plain=0):
        """(status, the six words, the checked layout's total); the words behind the array keep their pattern"""
        out = (C.c_int * 8)(*[PATTERN] * 8)
        checked = (C.c_int * 12)(*[PATTERN] * 12)
        rc_checked = C.c_int(-1)
        rc = L.emu_hoisted_sealed_layout(logn, Lq, K, dnum, plain, n_rot, out, checked, C.byref(rc_checked))
        assert list(out)[6:] == [PATTERN] * 2 and rc_checked.value == 0
        return rc, list(out)[:6], int(checked[11])
    return get


def checked_total(L, K, d, n_rot):
    """the checked hoisted rotations' block: shared intt_in [L], extend [d][M], ntt_ext [d][M]; per rotation mac [2][M], galois [2 M + L],
    intt_special [2][K], moddown [2][K + L], ntt_conv [2][L], tail [2][L]"""
    M = L + K
    return L + 2 * d * M + n_rot * (2 * M + 2 * M + L + 2 * K + 2 * (K + L) + 4 * L)


@pytest.mark.parametrize("n_rot", [1, 3])
def test_layout_is_c1_then_the_rotations_inputs_then_the_checked_block(layout, n_rot):
    for logn, L, K, dnum in PLANS:
        rc, out, inner = layout(logn, L, K, dnum, n_rot)
        per = L + dnum * 2 * (L + K)
        assert inner == checked_total(L, K, dnum, n_rot), (logn, L, K, dnum)
        assert rc == 0 and out == [0, L, per, L + n_rot * per, L + n_rot * per + inner, 1 if dnum <= CAP else 0], (logn, L, K, dnum)


def test_a_plan_with_a_plain_modulus_is_refused(layout):
    from fhe_reliability_gpu_amd._lib import lib
    for logn, L, K, dnum in PLANS:
        rc, out, _ = layout(logn, L, K, dnum, 3, plain=65537)
        assert rc == UNSUPPORTED and out == [PATTERN] * 6
        assert b"plain modulus" in lib.fhe_last_error()


def test_a_null_source_seal_is_refused(layout):
    """without the source's seal nothing would check the permutation: refused before tables or device are looked at, on a host-made
    context (emu_hoisted_sealed_layout.cpp), and the refused call takes an armed hook with it"""
    from fhe_reliability_gpu_amd._lib import lib
    so = C.CDLL(os.path.join(EMU_DIR, "libemu_hoisted_sealed_layout.so"))
    so.emu_sealed_null_source_seal.restype = C.c_int
    so.emu_sealed_null_source_seal.argtypes = [C.POINTER(C.c_int)]
    armed = C.c_int(-1)
    assert so.emu_sealed_null_source_seal(C.byref(armed)) == INVALID
    assert b"null seal" in lib.fhe_last_error() and armed.value == 0
