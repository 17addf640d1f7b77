"""Measurement tool: what verifying the diagonals on the load that multiplies them costs.  Timed with HIP events on one stream after
a warm-up, several rounds alternating in one process, on resident data.  50-bit ciphertext primes with 61-bit special primes, at
BASELINE config 4 (N = 2^17, L = 32, K = 8, dnum = 4) and config 5 (N = 2^16, L = 44, K = 11, dnum = 4) with n1 = n2 = 8; config 16
(N = 2^15, L = 8, K = 2, dnum = 2, n1 = 16, n2 = 2) reaches the inner sum's widest instantiation.
  (a) fhe_bsgs_matvec_sealed with every seal given, next to fhe_bsgs_matvec_checked and next to the four-part composition it
      replaces: fhe_seal_verify of c0, c1, every key and all diagonals, fhe_bsgs_matvec_checked, fhe_seal of both outputs.
  (b) the per-giant-step kernel pair on its own.  Neither has an entry point, so each is timed as a difference inside the same
      round: the product with n2 = 1 (baby block + one inner sum) minus the checked baby block alone.  Fused: the sealed call with
      only the diagonals' seals.  Composition: fhe_seal_verify over the step's n1 L diagonal rows plus the checked inner sum.  The
      fused inner sum moves about (3 n1 + 2) L N 8 bytes and the pair (4 n1 + 2) L N 8, so the byte count predicts
      (3 n1 + 2) / (4 n1 + 2) = 0.76 at n1 = 8; the seal kernels have so far run bound by integer work, not by bytes, so the ratio is
      reported, not promised.  The difference of two timed loops carries the noise of both, which the per-round figures show.
Before timing, the sealed call's words and output seals are held against the composition's on the same operands.
Reported, not gated.
python -m fhe_reliability_gpu_amd.tools.bsgs_sealed_rate [--config 4|5|16]"""
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
for cfg, logn, L, K, dnum, n1, n2 in _rate.configs(((4, 17, 32, 8, 4, 8, 8), (5, 16, 44, 11, 4, 8, 8), (16, 15, 8, 2, 2, 16, 2))):
    N, M = 1 << logn, L + K
    kr = dnum * 2 * M
    qs, t, ks, ab = _rate.plan(eng, logn, L, K, dnum)
    rnd, u64, _ = _rate.factories(min(qs))
    c0, c1, diags = rnd(L, N), rnd(L, N), rnd(n2, n1, L, N)
    y0, y1, z0, z1 = (torch.empty_like(c0) for _ in range(4))
    nb, ng = n1 - 1, n2 - 1
    bkeys, gkeys = [rnd(dnum, 2, M, N) for _ in range(nb)], [rnd(dnum, 2, M, N) for _ in range(ng)]      # any canonical words time the same
    be, ge = (C.c_uint32 * nb)(*[pow(5, b, 2 * N) for b in range(1, n1)]), (C.c_uint32 * ng)(*[pow(5, g * n1, 2 * N) for g in range(1, n2)])
    bk, gk = (vp * nb)(*[x.data_ptr() for x in bkeys]), (vp * ng)(*[x.data_ptr() for x in gkeys])
    r0, r1 = [torch.empty_like(c0) for _ in range(nb)], [torch.empty_like(c0) for _ in range(nb)]
    a0, a1 = (vp * nb)(*[x.data_ptr() for x in r0]), (vp * nb)(*[x.data_ptr() for x in r1])
    flags = torch.zeros(ks.bsgs_matvec_sealed_layout(n1, n2)["total"], dtype=torch.int32, device="cuda")
    cflags = torch.zeros(ks.bsgs_matvec_checked_layout(n1, n2)["total"], dtype=torch.int32, device="cuda")
    hflags = torch.zeros(ks.rotate_hoisted_checked_layout(nb)["total"], dtype=torch.int32, device="cuda")
    vflags = torch.zeros(max(n1 * n2 * L, kr), dtype=torch.int32, device="cuda")
    so, so2 = [u64(L, 2), u64(L, 2)], [u64(L, 2), u64(L, 2)]
    # the seals that travel with the operands, taken once
    seal = lambda words, n_poly, limbs: _rate.seal(eng, t, words, n_poly, limbs, sp)
    s_c, s_b, s_g, s_d = [seal(c0, 1, L), seal(c1, 1, L)], [seal(k, dnum * 2, M) for k in bkeys], [seal(k, dnum * 2, M) for k in gkeys], seal(diags, n1 * n2, L)
    sin, sout = (vp * 2)(*[x.data_ptr() for x in s_c]), (vp * 2)(*[x.data_ptr() for x in so])
    sbk, sgk = (vp * nb)(*[x.data_ptr() for x in s_b]), (vp * ng)(*[x.data_ptr() for x in s_g])

    def sealed(m=n2, every=True):
        check(lib.fhe_bsgs_matvec_sealed(h, ks._h, P(y0), P(y1), P(c0), P(c1), P(diags), n1, m, be, bk, ge, gk, ab._h, sin if every else None,
                                         sbk if every else None, sgk if every else None, P(s_d), sout if every else None, P(flags), sp))

    def checked(m=n2, o0=z0, o1=z1):
        check(lib.fhe_bsgs_matvec_checked(h, ks._h, P(o0), P(o1), P(c0), P(c1), P(diags), n1, m, be, bk, ge, gk, ab._h, P(cflags), sp))

    def verify(words, sl, n_poly, limbs):
        check(lib.fhe_seal_verify(h, P(words), P(sl), t._h, n_poly, limbs, 0, P(vflags), sp))

    def composition():
        verify(c0, s_c[0], 1, L)
        verify(c1, s_c[1], 1, L)
        for k, sl in zip(bkeys + gkeys, s_b + s_g):
            verify(k, sl, dnum * 2, M)
        verify(diags, s_d, n1 * n2, L)
        checked()
        for o, sl in zip((z0, z1), so2):
            check(lib.fhe_seal(h, P(sl), P(o), t._h, 1, L, 0, sp))

    baby_checked = lambda: check(lib.fhe_rotate_hoisted_checked(h, ks._h, a0, a1, P(c0), P(c1), be, bk, nb, ab._h, P(hflags), sp))
    verify_step = lambda: verify(diags[0], s_d, n1, L)
    name = f"config {cfg}: 2^{logn} L={L} K={K} dnum={dnum} n1={n1} n2={n2}"
    # the sealed call against the composition on the same operands: words, output seals, no flag
    sealed()
    composition()
    torch.cuda.synchronize()
    assert torch.equal(y0, z0) and torch.equal(y1, z1) and torch.equal(so[0], so2[0]) and torch.equal(so[1], so2[1]), f"{name}: the sealed call differs"
    where = {k: torch.nonzero(v).flatten()[:8].tolist() for k, v in (("sealed", flags), ("checked", cflags), ("verify", vflags)) if v.any()}
    assert not where, f"{name}: a clean run raised a flag (first words per buffer: {where})"
    reps, out = 5, []
    for r in range(3):
        ts, tc, tk = timed(sealed, reps), timed(composition, reps), timed(checked, reps)
        base = timed(baby_checked, reps)
        fused = timed(lambda: sealed(1, False), reps) - base
        inner = timed(lambda: checked(1), reps) - base
        sweep = timed(verify_step, reps)
        out.append((ts, tc, tk, fused, inner, sweep))
        print(f"{name} round {r}: sealed {ts:9.1f} us, composition {tc:9.1f} us ({ts / tc:.3f} x), checked {tk:9.1f} us ({ts / tk:.3f} x); per giant step "
              f"(by difference): fused inner sum {fused:7.1f} us, verifying sweep {sweep:7.1f} + checked inner sum {inner:7.1f} us "
              f"({fused / (sweep + inner):.3f} x, bytes predict {(3 * n1 + 2) / (4 * n1 + 2):.3f})", flush=True)
    torch.cuda.synchronize()
    assert not flags.any() and not cflags.any() and not hflags.any() and not vflags.any(), f"{name}: a clean run raised a flag"
    summary.append((name, med(out, lambda x: x[0] / x[1]), med(out, lambda x: x[3] / (x[5] + x[4]))))
    del ks, ab, c0, c1, diags, bkeys, gkeys, r0, r1
    torch.cuda.empty_cache()
print("summary (rounds with the median ratio):")
for name, a, b in summary:
    print(f"  {name}: sealed {a[0]:.1f} us, composition {a[1]:.1f} us: {a[0] / a[1]:.3f} x; checked {a[2]:.1f} us: {a[0] / a[2]:.3f} x the checked call")
    print(f"  {name}: per giant step, fused {b[3]:.1f} us, sweep {b[5]:.1f} + checked inner sum {b[4]:.1f} us: {b[3] / (b[5] + b[4]):.3f} x")
