"""Measurement tool: what the seal repair costs on clean rows.  Timed with HIP events on one stream after a warm-up, several rounds
alternating in one process, on resident data (the method of seal_rate.py).
  (a) fhe_seal_repair against fhe_seal_verify, and fhe_seal_locator against fhe_seal, over the 2 L rows of a two-part ciphertext at
      BASELINE config 4 (N = 2^17, L = 32) and config 5 (N = 2^16, L = 44).  On clean rows the repair adds one launch whose
      workgroups read a flag word and write a report record, so the ratio is expected near 1; the locator sweep reads the same
      bytes as fhe_seal with one more 61 x 32-bit product per word, so its ratio is expected near 1 as long as the sweep is bound
      by memory.
  (b) fhe_hmult_sealed_repair against fhe_hmult_sealed and fhe_rotate_sealed_repair against fhe_rotate_sealed at config 4 (K = 8,
      dnum = 4), CKKS form, all seals and locators given, output seals written; the repairing calls also write the output locators.
Reported, not gated.
python -m fhe_reliability_gpu_amd.tools.repair_rate [--skip-composites]"""
import ctypes as C
import sys

import torch

import fhe_reliability_gpu_amd as F
from fhe_reliability_gpu_amd._lib import check, lib, vp
from fhe_reliability_gpu_amd.tools import _rate
from fhe_reliability_gpu_amd.tools._rate import med

eng = F.Engine(0)
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
P = lambda x: C.c_void_p(x.data_ptr())
h = eng._h


timed = lambda fn, reps: _rate.timed(fn, reps, s, warmups=3)


u64 = lambda *shape: torch.zeros(shape, device="cuda", dtype=torch.int64)
_rate.print_device()
summary = []
for cfg, logn, L in ((4, 17, 32), (5, 16, 44)):
    N = 1 << logn
    qs = F.create_moduli(N, [50] * L)
    t = eng.tables(logn, qs)
    x = torch.randint(0, min(qs), (2, L, N), device="cuda", dtype=torch.int64)
    seal, loc, report = u64(2 * L, 2), u64(2 * L), u64(2 * L, 4)
    flags = torch.zeros(2 * L, device="cuda", dtype=torch.int32)
    torch.cuda.synchronize()      # the operands were written on torch's stream, the calls below run on `s`
    do_seal = lambda: check(lib.fhe_seal(h, P(seal), P(x), t._h, 2, L, 0, sp))
    do_loc = lambda: check(lib.fhe_seal_locator(h, P(loc), P(x), t._h, 2, L, 0, sp))
    verify = lambda: check(lib.fhe_seal_verify(h, P(x), P(seal), t._h, 2, L, 0, P(flags), sp))
    repair = lambda: check(lib.fhe_seal_repair(h, P(x), P(seal), P(loc), t._h, 2, L, 0, P(flags), P(report), sp))
    out = []
    for rnd in range(5):
        ts, tl, tv, tr = timed(do_seal, 50), timed(do_loc, 50), timed(verify, 50), timed(repair, 50)
        assert not flags.any() and not report.any(), "a clean repair raised a flag or reported an outcome"
        out.append((ts, tl, tv, tr))
        print(f"config {cfg} (N = 2^{logn}, {2 * L} rows) round {rnd}: fhe_seal {ts:7.1f} us, fhe_seal_locator {tl:7.1f} us ({tl / ts:.3f} x), "
              f"fhe_seal_verify {tv:7.1f} us, fhe_seal_repair {tr:7.1f} us ({tr / tv:.3f} x)", flush=True)
    _, tl, _, _ = med(out, lambda r: r[1] / r[0])
    ts = med(out, lambda r: r[1] / r[0])[0]
    tv, tr = med(out, lambda r: r[3] / r[2])[2:]
    nbytes = 2 * L * N * 8
    summary.append(f"config {cfg}: {nbytes / 2**20:.0f} MiB; fhe_seal_locator {tl:.1f} us = {tl / ts:.3f} x fhe_seal ({ts:.1f} us; {nbytes / tl / 1e6:.2f} TB/s); "
                   f"fhe_seal_repair on clean rows {tr:.1f} us = {tr / tv:.3f} x fhe_seal_verify ({tv:.1f} us; {tr - tv:+.1f} us)")
    del x, t

if "--skip-composites" not in sys.argv:
    logn, L, K, dnum = 17, 32, 8, 4
    N, M, R = 1 << logn, L + K, L - 1
    qs, t, ks, ab = _rate.plan(eng, logn, L, K, dnum)
    ops = [torch.randint(0, min(qs), (L, N), device="cuda", dtype=torch.int64) for _ in range(4)]
    key = torch.randint(0, min(qs), (dnum, 2, M, N), device="cuda", dtype=torch.int64)
    o0, o1 = u64(L, N), u64(L, N)
    sin, lin = [u64(L, 2) for _ in range(4)], [u64(L) for _ in range(4)]
    skey, lkey = u64(dnum * 2 * M, 2), u64(dnum * 2 * M)
    sout, lout = [u64(L, 2) for _ in range(2)], [u64(L) for _ in range(2)]
    torch.cuda.synchronize()
    for op, sl, ll in zip(ops, sin, lin):
        check(lib.fhe_seal(h, P(sl), P(op), t._h, 1, L, 0, sp))
        check(lib.fhe_seal_locator(h, P(ll), P(op), t._h, 1, L, 0, sp))
    check(lib.fhe_seal(h, P(skey), P(key), t._h, dnum * 2, M, 0, sp))
    check(lib.fhe_seal_locator(h, P(lkey), P(key), t._h, dnum * 2, M, 0, sp))
    a_sin, a_lin = (vp * 4)(*[x.data_ptr() for x in sin]), (vp * 4)(*[x.data_ptr() for x in lin])
    a_sout, a_lout = (vp * 2)(*[x.data_ptr() for x in sout]), (vp * 2)(*[x.data_ptr() for x in lout])
    hl, rl = ks.hmult_sealed_repair_layout(True), ks.rotate_sealed_repair_layout()
    flags = torch.zeros(max(hl["total"], rl["total"]), device="cuda", dtype=torch.int32)
    calls = {
        "fhe_hmult_sealed": lambda: check(lib.fhe_hmult_sealed(h, ks._h, P(o0), P(o1), *[P(x) for x in ops], P(key), 1, ab._h, a_sin, P(skey), a_sout, P(flags), sp)),
        "fhe_hmult_sealed_repair": lambda: check(lib.fhe_hmult_sealed_repair(h, ks._h, P(o0), P(o1), *[P(x) for x in ops], P(key), 1, ab._h, a_sin, a_lin, P(skey),
                                                                             P(lkey), a_sout, a_lout, P(flags), sp)),
        "fhe_rotate_sealed": lambda: check(lib.fhe_rotate_sealed(h, ks._h, P(o0), P(o1), P(ops[0]), P(ops[1]), 5, P(key), ab._h, a_sin, P(skey), a_sout, P(flags),
                                                                 sp)),
        "fhe_rotate_sealed_repair": lambda: check(lib.fhe_rotate_sealed_repair(h, ks._h, P(o0), P(o1), P(ops[0]), P(ops[1]), 5, P(key), ab._h, a_sin, a_lin,
                                                                               P(skey), P(lkey), a_sout, a_lout, P(flags), sp)),
    }
    for base, lay in (("fhe_hmult_sealed", hl), ("fhe_rotate_sealed", rl)):
        out = []
        for rnd in range(3):
            t0, t1 = timed(calls[base], 10), timed(calls[base + "_repair"], 10)
            assert not flags[:lay["flags_total"]].any() and not flags[lay["report"]:lay["total"]].any(), f"a clean {base}_repair raised a flag or reported an outcome"
            out.append((t0, t1))
            print(f"config 4 {base} round {rnd}: sealed {t0:8.1f} us, repairing {t1:8.1f} us ({t1 / t0:.3f} x)", flush=True)
        t0, t1 = med(out, lambda r: r[1] / r[0])
        summary.append(f"config 4 {base}_repair over {base}: {t0:.1f} us -> {t1:.1f} us ({t1 / t0:.3f} x), output locators included")
eng.check()
print("summary (median round):")
for line in summary:
    print("  " + line)
