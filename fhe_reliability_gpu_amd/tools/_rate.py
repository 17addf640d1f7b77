"""What the rate tools of this directory share -- not a tool itself, and importing it does not touch the GPU.  The measuring method
lives in timed(); the rest is what the sealed family's tools set up in the same way."""
import ctypes as C
import sys

import torch

import fhe_reliability_gpu_amd as F
from fhe_reliability_gpu_amd._lib import check, lib, vp

# (config, logn, L, K, dnum, plain modulus): BASELINE configs 4 and 5 in the CKKS form, the reference's shape in the BGV form
CONFIGS = ((4, 17, 32, 8, 4, 0), (5, 16, 44, 11, 4, 0), (14, 14, 4, 2, 2, 65537))


def timed(fn, reps, stream, warmups=2):
    """Mean device time of fn() in microseconds: warm-up calls, then a fresh pair of events on the tool's stream around every
    repetition, the host waiting for each."""
    for _ in range(warmups):
        fn()
    torch.cuda.synchronize()
    total = 0.0
    with torch.cuda.stream(stream):
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            total += a.elapsed_time(b)
    return total / reps * 1e3


def configs(table=CONFIGS):
    """the rows of a configuration table (config number first) that `--config N` on the command line selects: all without it"""
    only = int(sys.argv[sys.argv.index("--config") + 1]) if "--config" in sys.argv else 0
    return [row for row in table if not only or row[0] == only]


def plan(eng, logn, L, K, dnum, tp=0):
    """(qs, tables, KeySwitch, Abft): 50-bit ciphertext primes with 61-bit special primes, or all 50-bit with plain modulus tp"""
    qs = F.create_moduli(1 << logn, [50] * (L + K) if tp else [50] * L + [61] * K)
    t = eng.tables(logn, qs)
    ks, ab = F.KeySwitch(eng, t, L, K, dnum), F.Abft(eng, t)
    if tp:
        ks.set_plain_modulus(tp)
    return qs, t, ks, ab


def factories(lim):
    """(rnd, u64, i32): device tensors of random words below lim, of zero words, of zero flags"""
    rnd = lambda *shape: torch.randint(0, lim, shape, device="cuda", dtype=torch.int64)
    u64 = lambda *shape: torch.zeros(shape, device="cuda", dtype=torch.int64)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")
    return rnd, u64, i32


def seal(eng, t, words, n_poly, limbs, sp):
    """fhe_seal of words on the tool's stream sp, into a fresh tensor"""
    out = torch.zeros((n_poly * limbs, 2), device="cuda", dtype=torch.int64)
    torch.cuda.synchronize()          # torch fills on its own stream, the library writes on the tool's
    check(lib.fhe_seal(eng._h, C.c_void_p(out.data_ptr()), C.c_void_p(words.data_ptr()), t._h, n_poly, limbs, 0, sp))
    return out


ptrs = lambda xs: (vp * len(xs))(*[x.data_ptr() for x in xs])
med = lambda rows, key: sorted(rows, key=key)[len(rows) // 2]
spread = lambda rows, key: (min(key(r) for r in rows), max(key(r) for r in rows))


def print_device():
    print(f"device: {torch.cuda.get_device_name(0) or torch.cuda.get_device_properties(0).gcnArchName}")
