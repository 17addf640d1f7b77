"""Measurement tool: what sealing costs.  Timed with HIP events on one stream after a warm-up, several rounds alternating in one
process, on resident data.
  (a) fhe_seal and fhe_seal_verify over the 2 L rows of a two-part ciphertext at BASELINE config 4 (N = 2^17, L = 32) and config 5
      (N = 2^16, L = 44), next to fhe_modadd over the same rows.  A seal reads each word once; fhe_modadd reads two operands and
      writes one, three times the bytes, so the byte count predicts a ratio near 1/3.  Printed: the times, the measured ratio and
      the rate the seal's own bytes imply.
  (b) fhe_hmult_sealed over fhe_hmult_checked (CKKS form) and over fhe_bgv_hmult_checked (plain modulus 65537) at config 4
      (K = 8, dnum = 4), with all four operand seals, with and without the key seal, output seals written.  The key is
      dnum * 2 * (L + K) rows against an operand's L: its verification is expected to dominate what sealing adds.
Reported, not gated.
python -m fhe_reliability_gpu_amd.tools.seal_rate [--skip-hmult]"""
import ctypes as C
import sys

import torch

import fhe_reliability_gpu_amd as F
from fhe_reliability_gpu_amd._lib import check, lib, vp
from fhe_reliability_gpu_amd.tools import _rate
from fhe_reliability_gpu_amd.tools._rate import med

PLAIN_MODULUS = 65537
eng = F.Engine(0)
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
P = lambda x: C.c_void_p(x.data_ptr())
h = eng._h


timed = lambda fn, reps: _rate.timed(fn, reps, s, warmups=3)


_rate.print_device()
summary = []
for cfg, logn, L in ((4, 17, 32), (5, 16, 44)):
    N = 1 << logn
    qs = F.create_moduli(N, [50] * L)
    t = eng.tables(logn, qs)
    x, y = (torch.randint(0, min(qs), (2, L, N), device="cuda", dtype=torch.int64) for _ in range(2))
    z = torch.empty_like(x)
    seal = torch.zeros((2 * L, 2), device="cuda", dtype=torch.int64)
    flags = torch.zeros(2 * L, device="cuda", dtype=torch.int32)
    torch.cuda.synchronize()      # the operands were written on torch's stream, the calls below run on `s`
    add = lambda: check(lib.fhe_modadd(h, P(z), P(x), P(y), t._h, 2, L, 0, sp))
    do_seal = lambda: check(lib.fhe_seal(h, P(seal), P(x), t._h, 2, L, 0, sp))
    verify = lambda: check(lib.fhe_seal_verify(h, P(x), P(seal), t._h, 2, L, 0, P(flags), sp))
    out = []
    for rnd in range(5):
        ta, ts, tv = timed(add, 50), timed(do_seal, 50), timed(verify, 50)
        assert not flags.any(), "a clean verification raised a flag"
        out.append((ta, ts, tv))
        print(f"config {cfg} (N = 2^{logn}, {2 * L} rows) round {rnd}: fhe_modadd {ta:7.1f} us, fhe_seal {ts:7.1f} us ({ts / ta:.3f} x), "
              f"fhe_seal_verify {tv:7.1f} us ({tv / ta:.3f} x)", flush=True)
    ta, ts, tv = med(out, lambda r: r[1] / r[0])
    nbytes = 2 * L * N * 8
    summary.append(f"config {cfg}: {nbytes / 2**20:.0f} MiB sealed; fhe_modadd {ta:.1f} us ({3 * nbytes / ta / 1e6:.2f} TB/s over 3x the bytes), fhe_seal {ts:.1f} us "
                   f"= {ts / ta:.3f} x ({nbytes / ts / 1e6:.2f} TB/s), fhe_seal_verify {tv:.1f} us = {tv / ta:.3f} x ({nbytes / tv / 1e6:.2f} TB/s)")
    del x, y, z, t

if "--skip-hmult" not in sys.argv:
    logn, L, K, dnum = 17, 32, 8, 4
    N, M, R = 1 << logn, L + K, L - 1
    qs, t, ks, ab = _rate.plan(eng, logn, L, K, dnum)
    ops = [torch.randint(0, min(qs), (L, N), device="cuda", dtype=torch.int64) for _ in range(4)]
    rlk = torch.randint(0, min(qs), (dnum, 2, M, N), device="cuda", dtype=torch.int64)
    o0, o1 = (torch.empty((R, N), device="cuda", dtype=torch.int64) for _ in range(2))
    sin = [torch.zeros((L, 2), device="cuda", dtype=torch.int64) for _ in range(4)]
    skey = torch.zeros((dnum * 2 * M, 2), device="cuda", dtype=torch.int64)
    sout = [torch.zeros((R, 2), device="cuda", dtype=torch.int64) for _ in range(2)]
    torch.cuda.synchronize()      # the operands were written on torch's stream, the calls below run on `s`
    for op, sl in zip(ops, sin):
        check(lib.fhe_seal(h, P(sl), P(op), t._h, 1, L, 0, sp))
    check(lib.fhe_seal(h, P(skey), P(rlk), t._h, dnum * 2, M, 0, sp))
    a_in, a_out = (vp * 4)(*[x.data_ptr() for x in sin]), (vp * 2)(*[x.data_ptr() for x in sout])
    for form, tp in (("fhe_hmult_checked", 0), ("fhe_bgv_hmult_checked", PLAIN_MODULUS)):
        ks.set_plain_modulus(tp)
        lay = ks.hmult_sealed_layout(True)
        flags = torch.zeros(lay["total"], device="cuda", dtype=torch.int32)
        inner = lib.fhe_bgv_hmult_checked if tp else lib.fhe_hmult_checked
        checked = lambda: check(inner(h, ks._h, P(o0), P(o1), *[P(x) for x in ops], P(rlk), 1, ab._h, P(flags), sp))
        sealed = lambda key: check(lib.fhe_hmult_sealed(h, ks._h, P(o0), P(o1), *[P(x) for x in ops], P(rlk), 1, ab._h, a_in, P(skey) if key else None, a_out,
                                                        P(flags), sp))
        out = []
        for rnd in range(3):
            tc, t0, t1 = timed(checked, 10), timed(lambda: sealed(False), 10), timed(lambda: sealed(True), 10)
            assert not flags.any(), f"a clean sealed multiply raised flag words {flags.nonzero().flatten().tolist()[:8]} (layout {lay})"
            out.append((tc, t0, t1))
            print(f"config 4 {form} round {rnd}: checked {tc:8.1f} us, sealed without key seal {t0:8.1f} us ({t0 / tc:.3f} x), with key seal {t1:8.1f} us "
                  f"({t1 / tc:.3f} x)", flush=True)
        tc, t0, t1 = med(out, lambda r: r[2] / r[0])
        key_mb, op_mb = dnum * 2 * M * N * 8 / 2**20, (4 * L + 2 * R) * N * 8 / 2**20
        summary.append(f"config 4 fhe_hmult_sealed over {form}: {tc:.1f} us -> {t0:.1f} us ({t0 / tc:.3f} x) with the operands' and outputs' seals ({op_mb:.0f} MiB "
                       f"swept), {t1:.1f} us ({t1 / tc:.3f} x) with the key's as well ({key_mb:.0f} MiB more: {t1 - t0:.1f} us)")
eng.check()
print("summary (median round):")
for line in summary:
    print("  " + line)
