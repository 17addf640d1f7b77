"""Measurement tool: the round-to-nearest rescale (fhe_keyswitch_set_rescale_rounding, mode 1) against the flooring one (mode 0)
on the same plan, alternating in one process after a warm-up, timed with HIP events on one stream, on resident data:
fhe_rescale of two parts, and fhe_hmult with rescale on its default route.  Shapes on 50-bit ciphertext primes with 61-bit
special primes: BASELINE config 4 (N = 2^17, L = 32, K = 8), config 5 (N = 2^16, L = 44, K = 11), and N = 2^14, L = 4, K = 2.
The two modes run the same launches over the same bytes (the centring rides on a load both modes make; no launch is added), so
the bytes predict 1.0 x; the per-word arithmetic differs by a compare, a subtract and a select.  Median and spread over the
rounds are reported, not gated.
python -m fhe_reliability_gpu_amd.tools.rescale_round_rate [--config N]"""
import ctypes as C

import torch

import fhe_reliability_gpu_amd as F
from fhe_reliability_gpu_amd._lib import check, lib
from fhe_reliability_gpu_amd.tools import _rate

SHAPES = ((4, 17, 32, 8, 4), (5, 16, 44, 11, 4), (14, 14, 4, 2, 2))      # (config, logn, L, K, dnum); 14 = the small shape
ROUNDS, REPS = 5, 20
eng = F.Engine(0)
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
P = lambda x: C.c_void_p(x.data_ptr())

_rate.print_device()
summary = []
for cfg, logn, L, K, dnum in _rate.configs(SHAPES):
    N, M, R = 1 << logn, L + K, L - 1
    qs, t, ks, ab = _rate.plan(eng, logn, L, K, dnum)
    rnd, u64, _ = _rate.factories(min(qs))
    a0, a1, b0, b1 = (rnd(L, N) for _ in range(4))
    c, rlk = rnd(2, L, N), rnd(dnum, 2, M, N)
    o0, o1, ors = u64(R, N), u64(R, N), u64(2, R, N)
    torch.cuda.synchronize()
    rescale = lambda: check(lib.fhe_rescale(eng._h, ks._h, P(ors), P(c), 2, sp))
    hmult = lambda: check(lib.fhe_hmult(eng._h, ks._h, P(o0), P(o1), P(a0), P(a1), P(b0), P(b1), P(rlk), 1, sp))
    name = f"config {cfg}: 2^{logn} L={L} K={K} dnum={dnum}"
    rows = []
    for r in range(ROUNDS):
        row = []
        for fn in (rescale, hmult):
            for mode in (0, 1):
                ks.set_rescale_rounding(bool(mode))
                row.append(_rate.timed(fn, REPS, s, warmups=3))
        ks.set_rescale_rounding(False)
        rows.append(tuple(row))
        print(f"{name} round {r}: rescale floor {row[0]:8.1f} us, nearest {row[1]:8.1f} us ({row[1] / row[0]:.3f} x); "
              f"hmult floor {row[2]:8.1f} us, nearest {row[3]:8.1f} us ({row[3] / row[2]:.3f} x)", flush=True)
    summary.append((name, rows))
    del ks, ab, a0, a1, b0, b1, c, rlk, o0, o1, ors
print("summary (median ratio nearest / floor over the rounds, [min, max]):")
for name, rows in summary:
    rs, hm = (lambda r: r[1] / r[0]), (lambda r: r[3] / r[2])
    m_rs, m_hm = _rate.med(rows, rs), _rate.med(rows, hm)
    (rs_lo, rs_hi), (hm_lo, hm_hi) = _rate.spread(rows, rs), _rate.spread(rows, hm)
    print(f"  {name}: rescale {m_rs[0]:.1f} -> {m_rs[1]:.1f} us, {rs(m_rs):.3f} x [{rs_lo:.3f}, {rs_hi:.3f}]; "
          f"hmult {m_hm[2]:.1f} -> {m_hm[3]:.1f} us, {hm(m_hm):.3f} x [{hm_lo:.3f}, {hm_hi:.3f}]")
