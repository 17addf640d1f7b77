"""Every flag-layout call of the stage-by-stage checked composites against its closed form -- without a GPU.  The layout calls read
a plan's shape and nothing on the device, so tests/emu/emu_checked_layouts.cpp hands them a plan structure filled on the host.

The closed forms are the stage shapes the engine.py docstrings document, in order (M = L + K, d = dnum, R = L - 1, n = n_parts):
  key switch         intt_in [L], extend [d][M], ntt_ext [d][M], mac [2][M], intt_special [2][K], moddown [2][K + L], ntt_conv [2][L],
                     tail [2][L]; BGV then scale_special [2][K], scale_conv [2][L]
  rescale            intt_last [n], reduce [n][R], ntt_delta [n][R], scale [n][R]; BGV then scale_last [n], scale_delta [n][R]
  multiply           tensor [L][3], the key switch's block, the rescale's block for two parts (absent without rescale)
  hoisted rotations  shared intt_in, extend, ntt_ext; per rotation mac [2][M], galois [2 M + L], intt_special, moddown, ntt_conv, tail
  BSGS product       the baby block (hoisted rotations of n1 - 1 elements, absent for n1 = 1), then per giant step inner [2][L],
                     galois [2][L], add [L], the key switch's block
"""
import ctypes as C
import os
import subprocess
from itertools import accumulate

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
PKG = os.path.join(ROOT, "fhe_reliability_gpu_amd")
CSRC = os.path.join(PKG, "csrc")
OK, INVALID = 0, 1
PATTERN = 0x5A5A5A5A
KS, BGV_KS, RS, BGV_RS, HM, BGV_HM, HOISTED, BSGS = range(8)
WORDS = {KS: 10, BGV_KS: 12, RS: 6, BGV_RS: 8, HM: 4, BGV_HM: 4, HOISTED: 12, BSGS: 8}      # the arrays of include/fhe_mi355x.h
SHAPES = [(10, 4, 2, 2), (13, 3, 1, 3), (14, 6, 2, 3), (17, 32, 8, 4)]
PLAIN = 65537


@pytest.fixture(scope="module")
def layout():
    from fhe_reliability_gpu_amd import _lib      # the library the helper links against is loaded first
    so = os.path.join(EMU_DIR, "libemu_checked_layouts.so")
    srcs = [os.path.join(EMU_DIR, "emu_checked_layouts.cpp"), os.path.join(CSRC, "capi_internal.hpp"), os.path.join(CSRC, "fault_hook.hpp"), _lib.LIB_PATH]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call([hipcc, "-O1", "-std=c++17", "--cuda-host-only", "-x", "hip", "-shared", "-fPIC", "-I" + CSRC, srcs[0], "-L" + PKG,
                               "-lfhe_mi355x", "-Wl,-rpath," + PKG, "-o", so])
    L = C.CDLL(so)
    L.emu_checked_layout.restype = C.c_int
    L.emu_checked_layout.argtypes = [C.c_int] * 5 + [C.c_ulonglong, C.c_size_t, C.c_size_t, C.POINTER(C.c_int)]

    def get(which, shape, a=0, b=0):
        """(status, the call's whole array); the words behind the array keep their pattern"""
        out = (C.c_int * (WORDS[which] + 2))(*[PATTERN] * (WORDS[which] + 2))
        plain = PLAIN if which in (BGV_KS, BGV_RS, BGV_HM) else 0
        rc = L.emu_checked_layout(which, *shape, plain, a, b, out)
        assert list(out[WORDS[which]:]) == [PATTERN] * 2
        return rc, list(out[:WORDS[which]])
    return get


def offsets(sizes):
    """offsets of consecutive stages of these sizes, then their total"""
    return [0] + list(accumulate(sizes))


def ks_sizes(L, K, d):
    M = L + K
    return [L, d * M, d * M, 2 * M, 2 * K, 2 * (K + L), 2 * L, 2 * L]


def rs_sizes(L, n):
    R = L - 1
    return [n, n * R, n * R, n * R]


@pytest.mark.parametrize("shape", SHAPES)
def test_keyswitch_layouts(layout, shape):
    _, L, K, d = shape
    rc, ks = layout(KS, shape)
    # eight offsets, the total, one unused word
    assert rc == OK and ks == offsets(ks_sizes(L, K, d)) + [0]
    rc, bgv = layout(BGV_KS, shape)
    # stages 0-7, then 9 [2][K] and 10 [2][L], the total, one unused word
    assert rc == OK and bgv == offsets(ks_sizes(L, K, d) + [2 * K, 2 * L]) + [0]
    assert bgv[:8] == ks[:8] and bgv[8] == ks[8] and bgv[10] == ks[8] + 2 * K + 2 * L


@pytest.mark.parametrize("n_parts", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_rescale_layouts(layout, shape, n_parts):
    L, n = shape[1], n_parts
    rc, rs = layout(RS, shape, n)
    assert rc == OK and rs == offsets(rs_sizes(L, n)) + [0]
    rc, bgv = layout(BGV_RS, shape, n)
    # stages 0-3, then 4 [n] and 5 [n][R]
    assert rc == OK and bgv == offsets(rs_sizes(L, n) + [n, n * (L - 1)]) + [0]
    assert bgv[:4] == rs[:4] and bgv[4] == rs[4] and bgv[6] == rs[4] + n * L


@pytest.mark.parametrize("rescale", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_hmult_layouts(layout, shape, rescale):
    _, L, K, d = shape
    ks, rs = sum(ks_sizes(L, K, d)), sum(rs_sizes(L, 2))
    rc, hm = layout(HM, shape, rescale)
    assert rc == OK and hm == [0, 3 * L, 3 * L + ks, 3 * L + ks + (rs if rescale else 0)]
    rc, bgv = layout(BGV_HM, shape, rescale)
    ks_b, rs_b = ks + 2 * K + 2 * L, rs + 2 * L
    assert rc == OK and bgv == [0, 3 * L, 3 * L + ks_b, 3 * L + ks_b + (rs_b if rescale else 0)]


@pytest.mark.parametrize("n_rot", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_hoisted_layout(layout, shape, n_rot):
    _, L, K, d = shape
    M = L + K
    shared = offsets(ks_sizes(L, K, d)[:3])
    rot = offsets([2 * M, 2 * M + L, 2 * K, 2 * (K + L), 2 * L, 2 * L])
    rc, out = layout(HOISTED, shape, n_rot)
    # offsets of stages 0-2, of stages 3, 8, 4, 5, 6, 7 inside a rotation's block, the two block sizes, the total
    assert rc == OK and out == shared[:3] + rot[:6] + [shared[3], rot[6], shared[3] + n_rot * rot[6]]


@pytest.mark.parametrize("n1,n2", [(1, 1), (2, 2), (4, 2)])
@pytest.mark.parametrize("shape", SHAPES)
def test_bsgs_layout(layout, shape, n1, n2):
    _, L, K, d = shape
    M = L + K
    shared = sum(ks_sizes(L, K, d)[:3])
    rot = sum([2 * M, 2 * M + L, 2 * K, 2 * (K + L), 2 * L, 2 * L])
    baby = shared + (n1 - 1) * rot if n1 > 1 else 0
    giant = 5 * L + sum(ks_sizes(L, K, d))
    rc, out = layout(BSGS, shape, n1, n2)
    assert rc == OK and out == [0, baby, giant, 0, 2 * L, 4 * L, 5 * L, baby + n2 * giant]


def test_refusals(layout):
    one = (10, 1, 1, 1)      # L = 1: no prime left to drop
    for which in (RS, BGV_RS):
        assert layout(which, one, 1)[0] == INVALID
        for n_parts in (0, 4):
            assert layout(which, SHAPES[0], n_parts)[0] == INVALID
    for which in (HM, BGV_HM):
        assert layout(which, one, 1)[0] == INVALID
    # what drops no prime has a layout at L = 1
    K = d = 1
    ks = sum(ks_sizes(1, K, d))
    assert layout(KS, one) == (OK, offsets(ks_sizes(1, K, d)) + [0])
    assert layout(BGV_KS, one) == (OK, offsets(ks_sizes(1, K, d) + [2 * K, 2]) + [0])
    assert layout(HM, one, 0) == (OK, [0, 3, 3 + ks, 3 + ks])
    assert layout(BGV_HM, one, 0) == (OK, [0, 3, 3 + ks + 2 * K + 2, 3 + ks + 2 * K + 2])
