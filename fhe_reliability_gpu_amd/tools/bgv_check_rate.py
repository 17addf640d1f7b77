"""Measurement tool: the BGV forms of the checked key switch, mod switch and multiply (plans with a plain modulus), alternating in
one process after a warm-up, timed with HIP events on one stream, on resident data.  Two shapes: the reference's dot product
(N = 2^14, six 50-bit primes of which two are special: L = 4, K = 2, dnum = 2, dotprod_test.cu) and BASELINE config 4 (N = 2^17,
L = 32, K = 8, dnum = 4; 50-bit ciphertext primes, 61-bit special primes).  Two yardsticks per call:
  * the unchecked call on the same BGV plan (fhe_relinearize, fhe_rescale with two parts, fhe_hmult), with ks_fused = 0 and 1;
  * the existing checked call on the same plan with the plain modulus cleared -- what the two scalar stages add.  Byte count
    predicts 2 (K + L) rows of 16 N bytes for the key switch and n_parts L rows for the mod switch, printed next to their time at
    the 6.0 TB/s the transform passes sustain (bench.py FABRIC_SUSTAINED_GBS).
Reported, not gated.
python -m fhe_reliability_gpu_amd.tools.bgv_check_rate [--once] [--logn 14|17]
(--once: one BGV checked multiply per shape, for a kernel trace; --logn: that shape alone)"""
import ctypes as C
import sys

import torch

import fhe_reliability_gpu_amd as F
from fhe_reliability_gpu_amd._lib import check, lib
from fhe_reliability_gpu_amd.tools import _rate

FABRIC_SUSTAINED_GBS = 6000.0
PLAIN_MODULUS = 65537
eng = F.Engine(0)
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
P = lambda x: C.c_void_p(x.data_ptr())
ONCE = "--once" in sys.argv
ONLY = int(sys.argv[sys.argv.index("--logn") + 1]) if "--logn" in sys.argv else None


timed = lambda fn, reps: _rate.timed(fn, reps, s, warmups=3)


rows = []
for logn, L, K, dnum, sp_bits in ((14, 4, 2, 2, 50), (17, 32, 8, 4, 61)):
    if ONLY is not None and logn != ONLY:
        continue
    N, M, R = 1 << logn, L + K, L - 1
    qs = F.create_moduli(N, [50] * L + [sp_bits] * K)
    t = eng.tables(logn, qs)
    ks, ab = F.KeySwitch(eng, t, L, K, dnum), F.Abft(eng, t)
    lim = min(qs)
    a0, a1, b0, b1 = (torch.randint(0, lim, (L, N), device="cuda", dtype=torch.int64) for _ in range(4))
    c = torch.randint(0, lim, (2, L, N), device="cuda", dtype=torch.int64)
    rlk = torch.randint(0, lim, (dnum, 2, M, N), device="cuda", dtype=torch.int64)
    k0, k1 = torch.empty((L, N), device="cuda", dtype=torch.int64), torch.empty((L, N), device="cuda", dtype=torch.int64)
    o0, o1 = torch.empty((R, N), device="cuda", dtype=torch.int64), torch.empty((R, N), device="cuda", dtype=torch.int64)
    ors = torch.empty((2, R, N), device="cuda", dtype=torch.int64)
    flags = torch.zeros(ks.bgv_hmult_checked_layout(True)["total"], dtype=torch.int32, device="cuda")
    h = eng._h
    calls = {
        "keyswitch": (lambda: check(lib.fhe_relinearize(h, ks._h, P(k0), P(k1), P(a0), P(a1), P(b0), P(rlk), sp)),
                      lambda: check(lib.fhe_bgv_relinearize_checked(h, ks._h, P(k0), P(k1), P(a0), P(a1), P(b0), P(rlk), ab._h, P(flags), sp)),
                      lambda: check(lib.fhe_relinearize_checked(h, ks._h, P(k0), P(k1), P(a0), P(a1), P(b0), P(rlk), ab._h, P(flags), sp))),
        "mod_switch": (lambda: check(lib.fhe_rescale(h, ks._h, P(ors), P(c), 2, sp)),
                       lambda: check(lib.fhe_bgv_mod_switch_checked(h, ks._h, P(ors), P(c), 2, ab._h, P(flags), sp)),
                       lambda: check(lib.fhe_rescale_checked(h, ks._h, P(ors), P(c), 2, ab._h, P(flags), sp))),
        "hmult": (lambda: check(lib.fhe_hmult(h, ks._h, P(o0), P(o1), P(a0), P(a1), P(b0), P(b1), P(rlk), 1, sp)),
                  lambda: check(lib.fhe_bgv_hmult_checked(h, ks._h, P(o0), P(o1), P(a0), P(a1), P(b0), P(b1), P(rlk), 1, ab._h, P(flags), sp)),
                  lambda: check(lib.fhe_hmult_checked(h, ks._h, P(o0), P(o1), P(a0), P(a1), P(b0), P(b1), P(rlk), 1, ab._h, P(flags), sp))),
    }
    name = f"2^{logn} L={L} K={K} dnum={dnum}"
    ks.set_plain_modulus(PLAIN_MODULUS)
    if ONCE:
        calls["hmult"][1]()
        torch.cuda.synchronize()
        assert not flags.any()
        continue
    reps = 20
    for what, (plain, bgv, ckks) in calls.items():
        out = []
        for rnd in range(3):
            ks.set_plain_modulus(PLAIN_MODULUS)
            eng.set_option("ks_fused", 0)
            u0 = timed(plain, reps)
            eng.set_option("ks_fused", 1)
            u1 = timed(plain, reps)
            eng.set_option("ks_fused", -1)
            kb = timed(bgv, reps)
            assert not flags.any(), f"{name}: a clean BGV {what} raised a flag"
            ks.set_plain_modulus(0)
            kc = timed(ckks, reps)
            assert not flags.any(), f"{name}: a clean {what} raised a flag"
            out.append((u0, u1, kb, kc))
            print(f"{name} {what} round {rnd}: unchecked ks_fused=0 {u0:8.1f} us, ks_fused=1 {u1:8.1f} us, BGV checked {kb:8.1f} us "
                  f"({kb / u0:.3f} x, {kb / u1:.3f} x); checked without plain modulus {kc:8.1f} us ({kb / kc:.3f} x)", flush=True)
        rows_add = {"keyswitch": 2 * (K + L), "mod_switch": 2 * L, "hmult": 2 * (K + L) + 2 * L}[what]
        rows.append((name, what, rows_add * 16 * N) + sorted(out, key=lambda r: r[2] / r[3])[1])
    del ks, ab, a0, a1, b0, b1, c, rlk, k0, k1, o0, o1, ors
if not ONCE:
    print("summary (round with the median BGV-checked / checked ratio):")
    for name, what, own, u0, u1, kb, kc in rows:
        print(f"  {name} {what}: unchecked {u0:.1f} / {u1:.1f} us (ks_fused 0 / 1), BGV checked {kb:.1f} us: {kb / u0:.2f} x / {kb / u1:.2f} x; "
              f"checked without plain modulus {kc:.1f} us: {kb / kc:.3f} x; the scalar stages' own bytes {own / 1e6:.1f} MB = "
              f"{own / (FABRIC_SUSTAINED_GBS * 1e9) * 1e6:.1f} us at 6.0 TB/s")
