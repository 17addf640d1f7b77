"""Measurement tool: what verifying the multiply's operands on the load that multiplies them costs.  Timed with HIP events on one
stream after a warm-up, several rounds alternating in one process, on resident data.  50-bit ciphertext primes with 61-bit special
primes at BASELINE config 4 (N = 2^17, L = 32, K = 8, dnum = 4) and config 5 (N = 2^16, L = 44, K = 11, dnum = 4); the reference's
shape (N = 2^14, six 50-bit primes of which two special: L = 4, K = 2, dnum = 2, plain modulus 65537) in the BGV form.
  (a) fhe_tensor_product_sealed with and without output seals, next to the composition it replaces: 4 x fhe_seal_verify +
      fhe_tensor_product_checked (+ 3 x fhe_seal).  The sealed step moves 7 L N 8 bytes, the composition 11 (with output seals: 14),
      so the bytes predict 7 / 11 = 0.64 (7 / 14 = 0.50 with output seals); counting the tensor step's own 7 against 4 + 7 gives the
      56 / 88 of the same ratio.  The seal kernels have so far run bound by integer work, not by bytes: the ratio is reported, not
      promised.
  (b) fhe_hmult_sealed_fused against fhe_hmult_sealed, rescale on, every seal given.
Before timing, the sealed calls' words, output seals and flags are held against the composition's on the same operands.
Reported, not gated.
python -m fhe_reliability_gpu_amd.tools.tensor_sealed_rate [--config 4|5|14]"""
import ctypes as C

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


timed = lambda fn, reps: _rate.timed(fn, reps, s)


_rate.print_device()
summary = []
for cfg, logn, L, K, dnum, tp in _rate.configs():
    N, M = 1 << logn, L + K
    qs, t, ks, ab = _rate.plan(eng, logn, L, K, dnum, tp)
    rnd, u64, _ = _rate.factories(min(qs))
    ops = [rnd(L, N) for _ in range(4)]
    key = rnd(dnum, 2, M, N)                                    # any canonical words time the same
    d, e = [u64(L, N) for _ in range(3)], [u64(L, N) for _ in range(3)]
    so, so2 = [u64(L, 2) for _ in range(3)], [u64(L, 2) for _ in range(3)]
    flags, cflags, vflags = (torch.zeros(n, dtype=torch.int32, device="cuda") for n in (7 * L, 3 * L, 4 * L))
    hlay = ks.hmult_sealed_layout(True)
    hflags, hflags2 = (torch.zeros(hlay["total"], dtype=torch.int32, device="cuda") for _ in range(2))
    o, o2 = [u64(L - 1, N) for _ in range(2)], [u64(L - 1, N) for _ in range(2)]
    ho, ho2 = [u64(L - 1, 2) for _ in range(2)], [u64(L - 1, 2) for _ in range(2)]

    seal = lambda words, n_poly, limbs: _rate.seal(eng, t, words, n_poly, limbs, sp)
    s_ops, s_key = [seal(x, 1, L) for x in ops], seal(key, dnum * 2, M)
    sin = (vp * 4)(*[x.data_ptr() for x in s_ops])
    sout, hso, hso2 = (vp * 3)(*[x.data_ptr() for x in so]), (vp * 2)(*[x.data_ptr() for x in ho]), (vp * 2)(*[x.data_ptr() for x in ho2])

    def sealed(out=True):
        check(lib.fhe_tensor_product_sealed(h, P(d[0]), P(d[1]), P(d[2]), *[P(x) for x in ops], t._h, 1, L, 0, sin, sout if out else None, P(flags), sp))

    def composition(out=True):
        for i, (x, sl) in enumerate(zip(ops, s_ops)):
            check(lib.fhe_seal_verify(h, P(x), P(sl), t._h, 1, L, 0, P(vflags[i * L:]), sp))
        check(lib.fhe_tensor_product_checked(h, P(e[0]), P(e[1]), P(e[2]), *[P(x) for x in ops], t._h, L, 0, P(cflags), sp))
        for x, sl in zip(e, so2) if out else ():
            check(lib.fhe_seal(h, P(sl), P(x), t._h, 1, L, 0, sp))

    def hmult(call, outs, seals, fl):
        check(call(h, ks._h, P(outs[0]), P(outs[1]), *[P(x) for x in ops], P(key), 1, ab._h, sin, P(s_key), seals, P(fl), sp))

    fused = lambda: hmult(lib.fhe_hmult_sealed_fused, o, hso, hflags)
    swept = lambda: hmult(lib.fhe_hmult_sealed, o2, hso2, hflags2)
    name = f"config {cfg}: 2^{logn} L={L} K={K} dnum={dnum}" + (f" t={tp}" if tp else "")
    # the sealed calls against the compositions on the same operands: words, output seals, flags
    sealed()
    composition()
    fused()
    swept()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(d + so + o + ho, e + so2 + o2 + ho2)), f"{name}: a sealed call differs from its composition"
    assert torch.equal(hflags, hflags2), f"{name}: the fused multiply's flags differ"
    where = {k: torch.nonzero(v).flatten()[:8].tolist() for k, v in (("sealed", flags), ("checked", cflags), ("verify", vflags), ("hmult", hflags)) if v.any()}
    assert not where, f"{name}: a clean run raised a flag (first words per buffer: {where})"
    reps, out = 10, []
    for r in range(3):
        row = (timed(sealed, reps), timed(composition, reps), timed(lambda: sealed(False), reps), timed(lambda: composition(False), reps), timed(fused, reps),
               timed(swept, reps))
        out.append(row)
        print(f"{name} round {r}: tensor sealed {row[0]:8.1f} us, composition {row[1]:8.1f} us ({row[0] / row[1]:.3f} x, bytes predict {7 / 14:.3f}); without "
              f"output seals {row[2]:8.1f} / {row[3]:8.1f} us ({row[2] / row[3]:.3f} x, bytes predict {7 / 11:.3f}); hmult fused {row[4]:9.1f} us, swept "
              f"{row[5]:9.1f} us ({row[4] / row[5]:.3f} x)", flush=True)
    torch.cuda.synchronize()
    assert not flags.any() and not cflags.any() and not vflags.any() and not hflags.any() and not hflags2.any(), f"{name}: a clean run raised a flag"
    summary.append((name, med(out, lambda x: x[0] / x[1]), med(out, lambda x: x[2] / x[3]), med(out, lambda x: x[4] / x[5])))
    del ks, ab, ops, key, d, e, o, o2
    torch.cuda.empty_cache()
print("summary (rounds with the median ratio):")
for name, a, b, c in summary:
    print(f"  {name}: tensor sealed {a[0]:.1f} us vs 4 verify + checked + 3 seal {a[1]:.1f} us: {a[0] / a[1]:.3f} x")
    print(f"  {name}: without output seals {b[2]:.1f} us vs 4 verify + checked {b[3]:.1f} us: {b[2] / b[3]:.3f} x")
    print(f"  {name}: hmult_sealed_fused {c[4]:.1f} us vs hmult_sealed {c[5]:.1f} us: {c[4] / c[5]:.3f} x")
