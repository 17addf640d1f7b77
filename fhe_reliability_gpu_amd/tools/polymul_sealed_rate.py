"""Measurement tool: what verifying both factors of the negacyclic product on the loads that transform them and sealing the product
on its own store costs.  Timed with HIP events on one stream after a warm-up, several rounds alternating in one process at one
commit, on resident data.  Shapes: N = 2^16, 16 limbs x 16 polynomials (two-launch sizes: the sealed column passes around the
checked middle launch) and N = 2^12, 2 limbs x 64 polynomials (the single sealed launch), 50-bit primes.  Each with and without an
output seal:
  fhe_polymul_sealed against fhe_seal_verify(a) + fhe_seal_verify(b) + fhe_polymul_checked + fhe_seal(c)
  fhe_polymul_sealed without d_seal_c against fhe_seal_verify(a) + fhe_seal_verify(b) + fhe_polymul_checked
The byte count predicts one read each of a, b and c fewer than the composition, but the seal kernels have so far run bound by
integer work, not by bytes: the ratios are reported, not promised, and none is a pass condition.  Before timing, the new call's
words, output seal and flags are held against the composition's on the same operands.
python -m fhe_reliability_gpu_amd.tools.polymul_sealed_rate"""
import ctypes as C

import torch

import fhe_reliability_gpu_amd as F
from fhe_reliability_gpu_amd._lib import check, lib
from fhe_reliability_gpu_amd.tools import _rate
from fhe_reliability_gpu_amd.tools._rate import med, spread

eng = F.Engine(0)
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
P = lambda x: C.c_void_p(x.data_ptr())
h = eng._h

timed = lambda fn, reps: _rate.timed(fn, reps, s)

_rate.print_device()
summary = []
for logn, L, n_poly in ((16, 16, 16), (12, 2, 64)):
    N, rows = 1 << logn, L * n_poly
    qs = F.create_moduli(N, [50] * L)
    t = eng.tables(logn, qs)
    ab = F.Abft(eng, t)
    rnd, u64, i32 = _rate.factories(min(qs))
    a0, b0 = rnd(n_poly, L, N), rnd(n_poly, L, N)                # any canonical words time the same
    s_a, s_b = _rate.seal(eng, t, a0, n_poly, L, sp), _rate.seal(eng, t, b0, n_poly, L, sp)
    a, b, c, a2, b2, c2 = a0.clone(), b0.clone(), u64(n_poly, L, N), a0.clone(), b0.clone(), u64(n_poly, L, N)
    s_c, s_c2 = u64(rows, 2), u64(rows, 2)
    fl, fl2 = i32(5 * rows), i32(5 * rows)
    torch.cuda.synchronize()

    def sealed(out_seal=True):
        check(lib.fhe_polymul_sealed(h, P(c), P(a), P(b), t._h, ab._h, n_poly, L, 0, P(s_a), P(s_b), P(s_c) if out_seal else None, P(fl), sp))

    def composed(out_seal=True):
        check(lib.fhe_seal_verify(h, P(a2), P(s_a), t._h, n_poly, L, 0, P(fl2), sp))
        check(lib.fhe_seal_verify(h, P(b2), P(s_b), t._h, n_poly, L, 0, P(fl2[rows:]), sp))
        check(lib.fhe_polymul_checked(h, P(c2), P(a2), P(b2), t._h, ab._h, n_poly, L, 0, P(fl2[2 * rows:]), sp))
        if out_seal:
            check(lib.fhe_seal(h, P(s_c2), P(c2), t._h, n_poly, L, 0, sp))

    name = f"2^{logn} L={L} x {n_poly}"
    # the new call against the composition on the same operands: words, output seal, flags
    sealed()
    composed()
    torch.cuda.synchronize()
    assert torch.equal(c, c2) and torch.equal(s_c, s_c2) and torch.equal(fl, fl2) and not fl.any(), f"{name}: the sealed product differs from the composition"
    # the timed calls multiply what the last call left in the factors (scratch in both forms; at the single-launch size they are only
    # read); flags are not read
    calls = (sealed, composed, lambda: sealed(False), lambda: composed(False))
    reps, out = 10, []
    for r in range(5):
        row = tuple(timed(fn, reps) for fn in calls)
        out.append(row)
        print(f"{name} round {r}: polymul_sealed {row[0]:9.1f} us, verify + verify + checked + seal {row[1]:9.1f} us ({row[0] / row[1]:.3f} x); without an output "
              f"seal {row[2]:9.1f} us, verify + verify + checked {row[3]:9.1f} us ({row[2] / row[3]:.3f} x)", flush=True)
    summary.append((name, out))
    del t, ab, a0, b0, a, b, c, a2, b2, c2
    torch.cuda.empty_cache()
print("summary (round with the median ratio; spread of the ratio over the rounds):")
for name, out in summary:
    for what, base, i, j in (("polymul_sealed", "seal_verify x 2 + polymul_checked + seal", 0, 1),
                             ("polymul_sealed without an output seal", "seal_verify x 2 + polymul_checked", 2, 3)):
        ratio = lambda v: v[i] / v[j]
        m, (lo, hi) = med(out, ratio), spread(out, ratio)
        print(f"  {name}: {what} {m[i]:.1f} us vs {base} {m[j]:.1f} us: {ratio(m):.3f} x ({lo:.3f} .. {hi:.3f})")
