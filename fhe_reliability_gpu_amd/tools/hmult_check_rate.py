"""Measurement tool: the stage-by-stage checked rescale and the one-call checked homomorphic multiply against the unchecked calls,
alternating in one process after a warm-up, timed with HIP events on one stream, on resident data.  Two shapes on 50-bit
ciphertext primes with 61-bit special primes: N = 2^16, L = 16, K = 4, dnum = 4;  N = 2^17, L = 32, K = 8, dnum = 4 (BASELINE
config 4: multiply -> relinearize -> mod_switch_to_next, dotprod_test.cu:113-115).  Yardsticks, always the unchecked call:
fhe_rescale (two parts) for fhe_rescale_checked; fhe_hmult with hmult_fused_rescale = 0 (the three steps apart, as the checked
call runs them) and the default fhe_hmult (mod-down and rescale behind one forward transform) for fhe_hmult_checked.  The reduce
kernel's own bytes, (1 + R) n_parts N 8, are printed next to their time at the 6.0 TB/s the transform passes sustain (bench.py
FABRIC_SUSTAINED_GBS), to set against the kernel's line of a rocprofv3 --kernel-trace --stats run.  Reported, not gated.
python -m fhe_reliability_gpu_amd.tools.hmult_check_rate [--once] [--logn 16|17]
(--once: one checked multiply per shape, for a kernel trace; --logn: that shape alone, so that a trace holds one shape's launches)"""
import ctypes as C
import sys

import torch

import fhe_reliability_gpu_amd as F
from fhe_reliability_gpu_amd._lib import check, lib
from fhe_reliability_gpu_amd.tools import _rate

FABRIC_SUSTAINED_GBS = 6000.0
eng = F.Engine(0)
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
P = lambda x: C.c_void_p(x.data_ptr())
ONCE = "--once" in sys.argv
ONLY = int(sys.argv[sys.argv.index("--logn") + 1]) if "--logn" in sys.argv else None


timed = lambda fn, reps: _rate.timed(fn, reps, s, warmups=3)


rows = []
for logn, L, K, dnum in ((16, 16, 4, 4), (17, 32, 8, 4)):
    if ONLY is not None and logn != ONLY:
        continue
    N, M, R = 1 << logn, L + K, L - 1
    qs, t, ks, ab = _rate.plan(eng, logn, L, K, dnum)
    lim = min(qs)
    a0, a1, b0, b1 = (torch.randint(0, lim, (L, N), device="cuda", dtype=torch.int64) for _ in range(4))
    c = torch.randint(0, lim, (2, L, N), device="cuda", dtype=torch.int64)
    rlk = torch.randint(0, lim, (dnum, 2, M, N), device="cuda", dtype=torch.int64)
    o0, o1 = torch.empty((R, N), device="cuda", dtype=torch.int64), torch.empty((R, N), device="cuda", dtype=torch.int64)
    ors = torch.empty((2, R, N), device="cuda", dtype=torch.int64)
    flags = torch.zeros(ks.hmult_checked_layout(True)["total"], dtype=torch.int32, device="cuda")
    rs_plain = lambda: check(lib.fhe_rescale(eng._h, ks._h, P(ors), P(c), 2, sp))
    rs_checked = lambda: check(lib.fhe_rescale_checked(eng._h, ks._h, P(ors), P(c), 2, ab._h, P(flags), sp))
    hm_plain = lambda: check(lib.fhe_hmult(eng._h, ks._h, P(o0), P(o1), P(a0), P(a1), P(b0), P(b1), P(rlk), 1, sp))
    hm_checked = lambda: check(lib.fhe_hmult_checked(eng._h, ks._h, P(o0), P(o1), P(a0), P(a1), P(b0), P(b1), P(rlk), 1, ab._h, P(flags), sp))
    name = f"2^{logn} L={L} K={K} dnum={dnum}"
    if ONCE:
        hm_checked()
        torch.cuda.synchronize()
        assert not flags.any()
        continue
    reps, out = 20, []
    for rnd in range(3):
        ru = timed(rs_plain, reps)
        rk = timed(rs_checked, reps)
        assert not flags.any(), f"{name}: a clean rescale raised a flag"
        eng.set_option("hmult_fused_rescale", 0)
        hv = timed(hm_plain, reps)
        eng.set_option("hmult_fused_rescale", 1)
        hu = timed(hm_plain, reps)
        hk = timed(hm_checked, reps)
        out.append((ru, rk, hu, hv, hk))
        print(f"{name} round {rnd}: rescale {ru:8.1f} us, checked {rk:8.1f} us ({rk / ru:.3f} x); hmult {hu:8.1f} us, hmult_fused_rescale=0 {hv:8.1f} us, "
              f"checked {hk:8.1f} us ({hk / hu:.3f} x, {hk / hv:.3f} x)", flush=True)
    torch.cuda.synchronize()
    assert not flags.any(), f"{name}: a clean run raised a flag"
    own = (1 + R) * 2 * N * 8
    rows.append((name, own) + sorted(out, key=lambda r: r[4] / r[2])[1])
    del ks, ab, a0, a1, b0, b1, c, rlk, o0, o1, ors
if not ONCE:
    print("summary (round with the median hmult ratio):")
    for name, own, ru, rk, hu, hv, hk in rows:
        print(f"  {name}: rescale {ru:.1f} us, checked {rk:.1f} us: {rk / ru:.2f} x; hmult {hu:.1f} us, unfused {hv:.1f} us, checked {hk:.1f} us: "
              f"{hk / hu:.2f} x default, {hk / hv:.2f} x unfused; reduce kernel's own bytes {own / 1e6:.1f} MB = {own / (FABRIC_SUSTAINED_GBS * 1e9) * 1e6:.1f} us at 6.0 TB/s")
