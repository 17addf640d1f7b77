"""Measurement tool: the checked BSGS matrix-vector product against the unchecked one, its inner-sum kernel against the unchecked
kernel, and the checked add against the unchecked add; the calls alternate in one process after a warm-up, timed with HIP events on
one stream.  50-bit ciphertext primes with 61-bit special primes.  Three ratios:
  (a) fhe_bsgs_matvec_checked / fhe_bsgs_matvec (one stream, ntt_split off) at N = 2^16, L = 16, K = 4, dnum = 4, n1 = n2 = 4 and at
      N = 2^16, L = 44, K = 11, dnum = 4 (BASELINE config 5) with n1 = 4, n2 = 2
  (b) k_diag_mac_checked / k_diag_mac at the same shapes.  Neither kernel has an entry point of its own, so each is timed as a
      difference inside the same round: the product with n2 = 1 (baby block + one inner sum, nothing else) minus the baby block alone
      (fhe_rotate_hoisted / fhe_rotate_hoisted_checked with the same n1 - 1 elements).  The two kernels move the same bytes, so a ratio
      above 1 is arithmetic; the difference of two timed loops carries the noise of both, which the per-round figures show
  (c) fhe_modadd_checked / fhe_modadd on 16 polynomials of 16 limbs
Reported, not gated.
python -m fhe_reliability_gpu_amd.tools.bsgs_check_rate [--once]     (--once: one checked product per shape, for a kernel trace)"""
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
ONCE = "--once" in sys.argv


timed = lambda fn, reps: _rate.timed(fn, reps, s, warmups=3)


summary = []
for logn, L, K, dnum, n1, n2 in ((16, 16, 4, 4, 4, 4), (16, 44, 11, 4, 4, 2)):
    N, M = 1 << logn, L + K
    qs, t, ks, ab = _rate.plan(eng, logn, L, K, dnum)
    lim = min(qs)
    rnd = lambda *shape: torch.randint(0, lim, shape, device="cuda", dtype=torch.int64)
    c0, c1, diags = rnd(L, N), rnd(L, N), rnd(n2, n1, L, N)
    y0, y1 = torch.empty_like(c0), torch.empty_like(c0)
    nb, ng = n1 - 1, n2 - 1
    bkeys, gkeys = [rnd(dnum, 2, M, N) for _ in range(nb)], [rnd(dnum, 2, M, N) for _ in range(ng)]      # any canonical words time the same
    be, ge = (C.c_uint32 * nb)(*[pow(5, b, 2 * N) for b in range(1, n1)]), (C.c_uint32 * ng)(*[pow(5, g * n1, 2 * N) for g in range(1, n2)])
    bk, gk = (vp * nb)(*[x.data_ptr() for x in bkeys]), (vp * ng)(*[x.data_ptr() for x in gkeys])
    r0, r1 = [torch.empty_like(c0) for _ in range(nb)], [torch.empty_like(c0) for _ in range(nb)]
    a0, a1 = (vp * nb)(*[x.data_ptr() for x in r0]), (vp * nb)(*[x.data_ptr() for x in r1])
    flags = torch.zeros(ks.bsgs_matvec_checked_layout(n1, n2)["total"], dtype=torch.int32, device="cuda")
    hflags = torch.zeros(ks.rotate_hoisted_checked_layout(nb)["total"], dtype=torch.int32, device="cuda")
    plain = lambda m=n2: check(lib.fhe_bsgs_matvec(eng._h, ks._h, P(y0), P(y1), P(c0), P(c1), P(diags), n1, m, be, bk, ge, gk, sp))
    checked = lambda m=n2: check(lib.fhe_bsgs_matvec_checked(eng._h, ks._h, P(y0), P(y1), P(c0), P(c1), P(diags), n1, m, be, bk, ge, gk, ab._h, P(flags), sp))
    baby = lambda: check(lib.fhe_rotate_hoisted(eng._h, ks._h, a0, a1, P(c0), P(c1), be, bk, nb, sp))
    baby_checked = lambda: check(lib.fhe_rotate_hoisted_checked(eng._h, ks._h, a0, a1, P(c0), P(c1), be, bk, nb, ab._h, P(hflags), sp))
    name = f"2^{logn} L={L} K={K} dnum={dnum} n1={n1} n2={n2}"
    if ONCE:
        checked()
        torch.cuda.synchronize()
        assert not flags.any()
        continue
    eng.set_option("ntt_split", 0)          # the unchecked baby rotations on one stream, as the checked ones run
    reps, out = 10, []
    for r in range(3):
        u, c = timed(plain, reps), timed(checked, reps)
        du = timed(lambda: plain(1), reps) - timed(baby, reps)
        dc = timed(lambda: checked(1), reps) - timed(baby_checked, reps)
        out.append((u, c, du, dc))
        print(f"{name} round {r}: bsgs_matvec {u:8.1f} us, checked {c:8.1f} us ({c / u:.3f} x); inner sum alone (by difference) {du:6.1f} us, "
              f"checked {dc:6.1f} us ({dc / du:.3f} x)", flush=True)
    eng.set_option("ntt_split", -1)
    torch.cuda.synchronize()
    assert not flags.any() and not hflags.any(), f"{name}: a clean run raised a flag"
    summary.append((name, med(out, lambda x: x[1] / x[0])[:2], med(out, lambda x: x[3] / x[2])[2:]))
    del ks, ab, c0, c1, diags, bkeys, gkeys, r0, r1
if not ONCE:
    # (c) the add alone: 16 polynomials of 16 limbs at N = 2^16
    logn, L, n_poly = 16, 16, 16
    N = 1 << logn
    qs = F.create_moduli(N, [50] * L)
    t = eng.tables(logn, qs)
    a, b = (torch.randint(0, min(qs), (n_poly, L, N), device="cuda", dtype=torch.int64) for _ in range(2))
    c = torch.empty_like(a)
    fl = torch.zeros(n_poly * L, dtype=torch.int32, device="cuda")
    add = lambda: check(lib.fhe_modadd(eng._h, P(c), P(a), P(b), t._h, n_poly, L, 0, sp))
    add_checked = lambda: check(lib.fhe_modadd_checked(eng._h, P(c), P(a), P(b), t._h, n_poly, L, 0, P(fl), sp))
    adds = []
    for r in range(3):
        u, k = timed(add, 40), timed(add_checked, 40)
        adds.append((u, k))
        print(f"modadd 2^16 {n_poly} x L={L} round {r}: {u:6.1f} us, checked {k:6.1f} us ({k / u:.3f} x)", flush=True)
    torch.cuda.synchronize()
    assert not fl.any()
    print("summary (rounds with the median ratio):")
    for name, (u, c), (du, dc) in summary:
        print(f"  {name}: bsgs_matvec {u:.1f} us, checked {c:.1f} us: {c / u:.2f} x; inner sum alone {du:.1f} us, checked {dc:.1f} us: {dc / du:.2f} x")
    u, k = med(adds, lambda x: x[1] / x[0])
    print(f"  modadd 2^16 {n_poly} x L={L}: {u:.1f} us, checked {k:.1f} us: {k / u:.2f} x")
