"""Measurement tool: the stage-by-stage checked key switch against the unchecked one, the calls alternating in one process after
a warm-up, timed with HIP events on one stream.  Three shapes on 50-bit ciphertext primes with 61-bit special primes:
N = 2^16, L = 16, K = 4, dnum = 4;  N = 2^16, L = 44, K = 11, dnum = 4 (BASELINE config 5);  N = 2^17, L = 32, K = 8, dnum = 4
(config 4, the relinearisation's key switch).  Two yardsticks per shape: the default unchecked call, and the unchecked call with
ks_fused = 0 (the inner product as a launch of its own, as the checked call runs it) -- the fused mod-down tail stays on in both.
Reported, not gated.
python -m fhe_reliability_gpu_amd.tools.keyswitch_check_rate [--once]     (--once: one checked call per shape, for a kernel trace)"""
import ctypes as C
import sys

import torch

import fhe_reliability_gpu_amd as F
from fhe_reliability_gpu_amd._lib import check, lib
from fhe_reliability_gpu_amd.tools import _rate

eng = F.Engine(0)
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
P = lambda x: C.c_void_p(x.data_ptr())
ONCE = "--once" in sys.argv


timed = lambda fn, reps: _rate.timed(fn, reps, s, warmups=3)


rows = []
for logn, L, K, dnum in ((16, 16, 4, 4), (16, 44, 11, 4), (17, 32, 8, 4)):
    N, M = 1 << logn, L + K
    qs, t, ks, ab = _rate.plan(eng, logn, L, K, dnum)
    lim = min(qs)
    c = torch.randint(0, lim, (L, N), device="cuda", dtype=torch.int64)
    evk = torch.randint(0, lim, (dnum, 2, M, N), device="cuda", dtype=torch.int64)
    o0, o1 = torch.empty_like(c), torch.empty_like(c)
    flags = torch.zeros(ks.checked_layout()["total"], dtype=torch.int32, device="cuda")
    plain = lambda: check(lib.fhe_keyswitch_apply(eng._h, ks._h, P(o0), P(o1), P(c), P(evk), sp))
    checked = lambda: check(lib.fhe_keyswitch_apply_checked(eng._h, ks._h, P(o0), P(o1), P(c), P(evk), None, None, ab._h, P(flags), sp))
    name = f"2^{logn} L={L} K={K} dnum={dnum}"
    if ONCE:
        checked()
        torch.cuda.synchronize()
        assert not flags.any()
        continue
    reps, out = 20, []
    for rnd in range(3):
        eng.set_option("ks_fused", -1)
        u = timed(plain, reps)
        eng.set_option("ks_fused", 0)
        v = timed(plain, reps)
        eng.set_option("ks_fused", -1)
        k = timed(checked, reps)
        out.append((u, v, k))
        print(f"{name} round {rnd}: unchecked {u:8.1f} us, unchecked ks_fused=0 {v:8.1f} us, checked {k:8.1f} us ({k / u:.3f} x, {k / v:.3f} x)", flush=True)
    torch.cuda.synchronize()
    assert not flags.any(), f"{name}: a clean run raised a flag"
    rows.append((name,) + sorted(out, key=lambda r: r[2] / r[0])[1])
    del ks, ab, c, evk, o0, o1
if not ONCE:
    print("summary (round with the median ratio):")
    for name, u, v, k in rows:
        print(f"  {name}: unchecked {u:.1f} us, unchecked ks_fused=0 {v:.1f} us, checked {k:.1f} us: {k / u:.2f} x default, {k / v:.2f} x unfused")
