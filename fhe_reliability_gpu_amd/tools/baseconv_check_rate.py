"""Measurement tool: the residue-checked base conversions against the unchecked ones, checked and unchecked calls alternating
in one process, at the two key-switch shapes -- N = 2^16 with m = 11 -> k = 44 and N = 2^17 with m = 8 -> k = 32 -- on 50-bit
primes (the plan's FP64 path) and with a 61-bit prime among the inputs (the integer path), and the fast form at the second
shape on 50-bit primes.  Reported, not gated.
python -m fhe_reliability_gpu_amd.tools.baseconv_check_rate"""
import ctypes as C

import torch

import fhe_reliability_gpu_amd as F
from fhe_reliability_gpu_amd._lib import check, lib
from fhe_reliability_gpu_amd.tools import _rate

eng = F.Engine(0)
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
P = lambda x: C.c_void_p(x.data_ptr())


timed = lambda fn, reps: _rate.timed(fn, reps, s, warmups=3)


def compare(name, plain, checked, flags, reps=50, rounds=3):
    out = []
    for rnd in range(rounds):
        u, c = timed(plain, reps), timed(checked, reps)
        out.append((u, c))
        print(f"{name} round {rnd}: unchecked {u:7.1f} us, checked {c:7.1f} us ({c / u:.3f} x)", flush=True)
    torch.cuda.synchronize()
    assert not flags.any(), f"{name}: a clean run raised a flag"
    u, c = sorted(out, key=lambda p: p[1] / p[0])[rounds // 2]
    return u, c


rows = []
for logn, m, k in ((16, 11, 44), (17, 8, 32)):
    N = 1 << logn
    for big in (False, True):
        qs = F.create_moduli(N, [50] * (m + k - 1) + [61 if big else 50])
        qs = qs[-1:] + qs[:-1] if big else qs
        mi, mo = qs[:m], qs[m:]
        bc = F.BaseConv(eng, mi, mo)
        x = torch.stack([torch.randint(0, p, (N,), device="cuda", dtype=torch.int64) for p in mi])
        out = torch.empty((k, N), device="cuda", dtype=torch.int64)
        flags = torch.zeros(m + k, dtype=torch.int32, device="cuda")
        name = f"exact 2^{logn} {m}->{k} {'61-bit (integer plan)' if big else '50-bit (FP64 plan)'}"
        rows.append((name,) + compare(name,
                                      lambda: check(lib.fhe_baseconv_exact(eng._h, P(out), P(x), bc._h, N, sp)),
                                      lambda: check(lib.fhe_baseconv_exact_checked(eng._h, P(out), P(x), bc._h, N, P(flags), sp)), flags))
        if logn == 17 and not big:
            name = f"fast 2^{logn} {m}->{k} 50-bit"
            rows.append((name,) + compare(name,
                                          lambda: check(lib.fhe_baseconv_fast(eng._h, P(out), P(x), bc._h, N, sp)),
                                          lambda: check(lib.fhe_baseconv_fast_checked(eng._h, P(out), P(x), bc._h, N, P(flags), sp)), flags))
        del bc, x, out
print("summary (round with the median ratio):")
for name, u, c in rows:
    print(f"  {name}: unchecked {u:.1f} us, checked {c:.1f} us, {c / u:.2f} x")
