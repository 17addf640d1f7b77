"""Measurement tool: checked hoisted rotations against the unchecked ones and against one checked rotation per element, and the
checked Galois permutation against the unchecked one; the calls alternate in one process after a warm-up, timed with HIP events on
one stream.  Two shapes on 50-bit ciphertext primes with 61-bit special primes, 8 rotations each: N = 2^16, L = 16, K = 4,
dnum = 4 and N = 2^16, L = 44, K = 11, dnum = 4 (BASELINE config 5).  Three ratios per shape:
  checked hoisted per rotation / fhe_rotate_hoisted per rotation on one stream (ntt_split off)
  checked hoisted per rotation / fhe_rotate_checked
  fhe_automorphism_ntt_checked / fhe_automorphism_ntt on 2 (L + K) + L rows of N words (one rotation's permutation stage)
Reported, not gated.
python -m fhe_reliability_gpu_amd.tools.hoisted_check_rate [--once]     (--once: one checked hoisted call per shape, for a kernel trace)"""
import ctypes as C
import sys

import torch

import fhe_reliability_gpu_amd as F
from fhe_reliability_gpu_amd._lib import check, lib, vp
from fhe_reliability_gpu_amd.tools import _rate

eng = F.Engine(0)
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
P = lambda x: C.c_void_p(x.data_ptr())
ONCE = "--once" in sys.argv
N_ROT = 8


timed = lambda fn, reps: _rate.timed(fn, reps, s, warmups=3)


rows = []
for logn, L, K, dnum in ((16, 16, 4, 4), (16, 44, 11, 4)):
    N, M = 1 << logn, L + K
    qs, t, ks, ab = _rate.plan(eng, logn, L, K, dnum)
    lim = min(qs)
    rnd = lambda *shape: torch.randint(0, lim, shape, device="cuda", dtype=torch.int64)
    c0, c1 = rnd(L, N), rnd(L, N)
    elts = [pow(5, i + 1, 2 * N) for i in range(N_ROT)]
    keys = [rnd(dnum, 2, M, N) for _ in range(N_ROT)]          # stand-ins for prepared keys: any canonical words time the same
    o0, o1 = [torch.empty_like(c0) for _ in range(N_ROT)], [torch.empty_like(c0) for _ in range(N_ROT)]
    a0, a1 = (vp * N_ROT)(*[x.data_ptr() for x in o0]), (vp * N_ROT)(*[x.data_ptr() for x in o1])
    pk, ge = (vp * N_ROT)(*[x.data_ptr() for x in keys]), (C.c_uint32 * N_ROT)(*elts)
    hflags = torch.zeros(ks.rotate_hoisted_checked_layout(N_ROT)["total"], dtype=torch.int32, device="cuda")
    rflags = torch.zeros(ks.checked_layout()["total"], dtype=torch.int32, device="cuda")
    rows_g = 2 * M + L
    gsrc, gdst = rnd(rows_g, N), torch.empty(rows_g, N, device="cuda", dtype=torch.int64)
    gflags = torch.zeros(rows_g, dtype=torch.int32, device="cuda")
    hoisted = lambda: check(lib.fhe_rotate_hoisted(eng._h, ks._h, a0, a1, P(c0), P(c1), ge, pk, N_ROT, sp))
    hoisted_checked = lambda: check(lib.fhe_rotate_hoisted_checked(eng._h, ks._h, a0, a1, P(c0), P(c1), ge, pk, N_ROT, ab._h, P(hflags), sp))
    rotate_checked = lambda: check(lib.fhe_rotate_checked(eng._h, ks._h, P(o0[0]), P(o1[0]), P(c0), P(c1), elts[0], P(keys[0]), ab._h, P(rflags), sp))
    perm = lambda: check(lib.fhe_automorphism_ntt(eng._h, P(gdst), P(gsrc), logn, elts[0], rows_g, sp))
    perm_checked = lambda: check(lib.fhe_automorphism_ntt_checked(eng._h, P(gdst), P(gsrc), logn, elts[0], rows_g, P(gflags), sp))
    name = f"2^{logn} L={L} K={K} dnum={dnum} n_rot={N_ROT}"
    if ONCE:
        hoisted_checked()
        torch.cuda.synchronize()
        assert not hflags.any()
        continue
    eng.set_option("ntt_split", 0)          # the unchecked hoisted rotations on one stream, as the checked ones run
    reps, out = 10, []
    for r in range(3):
        u = timed(hoisted, reps) / N_ROT
        h = timed(hoisted_checked, reps) / N_ROT
        k = timed(rotate_checked, reps)
        g, gc = timed(perm, 4 * reps), timed(perm_checked, 4 * reps)
        out.append((u, h, k, g, gc))
        print(f"{name} round {r}: per rotation: hoisted {u:7.1f} us, checked hoisted {h:7.1f} us ({h / u:.3f} x), fhe_rotate_checked {k:7.1f} us "
              f"({h / k:.3f} x); permutation of {rows_g} rows: {g:6.1f} us, checked {gc:6.1f} us ({gc / g:.3f} x)", flush=True)
    eng.set_option("ntt_split", -1)
    torch.cuda.synchronize()
    assert not hflags.any() and not rflags.any() and not gflags.any(), f"{name}: a clean run raised a flag"
    rows.append((name,) + sorted(out, key=lambda x: x[1] / x[2])[1])
    del ks, ab, c0, c1, keys, o0, o1, gsrc, gdst
if not ONCE:
    print("summary (round with the median checked-hoisted / checked-rotation ratio):")
    for name, u, h, k, g, gc in rows:
        print(f"  {name}: per rotation hoisted {u:.1f} us, checked hoisted {h:.1f} us, fhe_rotate_checked {k:.1f} us: {h / u:.2f} x hoisted, "
              f"{h / k:.2f} x checked rotation; permutation {g:.1f} us, checked {gc:.1f} us: {gc / g:.2f} x")
