"""How the CPU emulation tests build and load their library: one g++ line, rebuilt when the library is missing or older than any
source or dependency.  Every tests/test_emu_*.py keeps its own ``emu`` fixture -- the call below plus its restype / argtypes lines."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "fhe_reliability_gpu_amd", "csrc")
# -ffp-contract=off: the emulation's FP64 products round as the kernels' do, never fused into an fma by the host compiler
DEFAULT_FLAGS = ("-O2", "-std=c++17", "-ffp-contract=off")


def build_emu(lib_name, sources, deps, flags=DEFAULT_FLAGS):
    """the loaded CDLL of tests/emu/<lib_name>: ``sources`` (names under tests/emu, or absolute paths) are compiled, ``deps`` (names
    under csrc, or absolute paths) only dated; ``flags`` go between ``g++`` and ``-shared -fPIC -I<csrc>``"""
    so = os.path.join(EMU_DIR, lib_name)
    sources = [os.path.join(EMU_DIR, s) for s in sources]
    dated = sources + [os.path.join(CSRC, d) for d in deps]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in dated):
        subprocess.check_call(["g++", *flags, "-shared", "-fPIC", "-I" + CSRC, *sources, "-o", so])
    return C.CDLL(so)
