"""Measurement tool: what verifying the forward transform's input on its own load and sealing its output on its own store costs.
Timed with HIP events on one stream after a warm-up, several rounds alternating in one process at one commit, on resident data.
L rows of 50-bit primes at BASELINE config 4 (N = 2^17, L = 32), config 5 (N = 2^16, L = 44) and the reference's shape (N = 2^14,
L = 4).  Each new call next to the composition it replaces:
  (a) fhe_ntt_forward_sealed in place against fhe_seal_verify + fhe_ntt_forward_checked + fhe_seal in place;
  (b) fhe_ntt_forward_sealed out of place against the same composition behind a device copy;
  (c) fhe_ntt_inverse_sealed_out out of place against fhe_ntt_inverse_sealed + fhe_seal.
The byte count predicts 32 N against 48 N per row for (a), 0.67 x, but the seal kernels have so far run bound by integer work, not
by bytes: the ratios are reported, not promised, and none is a pass condition.  Before timing, the new calls' words, output seals
and flags are held against their baselines' on the same operands.
python -m fhe_reliability_gpu_amd.tools.ntt_fwd_sealed_rate [--config 4|5|14]"""
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
for cfg, logn, L, _, _, _ in _rate.configs():
    N = 1 << logn
    qs = F.create_moduli(N, [50] * L)
    t = eng.tables(logn, qs)
    ab = F.Abft(eng, t)
    rnd, u64, i32 = _rate.factories(min(qs))
    x = rnd(L, N)                                               # any canonical words time the same
    s_x = _rate.seal(eng, t, x, 1, L, sp)
    work, work2, dst, dst2 = x.clone(), x.clone(), u64(L, N), u64(L, N)
    X, iout, iout2 = u64(L, N), u64(L, N), u64(L, N)
    so, so2, sX, si, si2 = (u64(L, 2) for _ in range(5))
    fl, fl2, ifl, ifl2 = (i32(2 * L) for _ in range(4))
    torch.cuda.synchronize()

    def fwd_sealed(d, src, seal_dst, flags):
        check(lib.fhe_ntt_forward_sealed(h, P(d), P(src), t._h, ab._h, 1, L, 0, P(s_x), P(seal_dst), P(flags), sp))

    def fwd_composed(d, seal_dst, flags, copy):
        if copy:
            check(lib.fhe_d2d(h, P(d), P(x), L * N * 8, sp))
        check(lib.fhe_seal_verify(h, P(d), P(s_x), t._h, 1, L, 0, P(flags), sp))
        check(lib.fhe_ntt_forward_checked(h, P(d), t._h, ab._h, 1, L, 0, P(flags[L:]), sp))
        check(lib.fhe_seal(h, P(seal_dst), P(d), t._h, 1, L, 0, sp))

    def inv_sealed_out():
        check(lib.fhe_ntt_inverse_sealed_out(h, P(iout), P(X), t._h, ab._h, 1, L, 0, P(sX), P(si), P(ifl), sp))

    def inv_composed():
        check(lib.fhe_ntt_inverse_sealed(h, P(iout2), P(X), t._h, ab._h, 1, L, 0, P(sX), P(ifl2), sp))
        check(lib.fhe_seal(h, P(si2), P(iout2), t._h, 1, L, 0, sp))

    name = f"config {cfg}: 2^{logn} L={L}"
    # the new calls against their baselines on the same operands: words, output seals, flags
    fwd_sealed(dst, x, so, fl)
    fwd_composed(dst2, so2, fl2, True)
    torch.cuda.synchronize()
    assert torch.equal(dst, dst2) and torch.equal(so, so2) and torch.equal(fl, fl2) and not fl.any(), f"{name}: the sealed forward transform differs from the composition"
    X.copy_(dst)
    sX.copy_(so)
    torch.cuda.synchronize()
    inv_sealed_out()
    inv_composed()
    torch.cuda.synchronize()
    assert torch.equal(iout, x) and torch.equal(iout, iout2) and torch.equal(si, si2) and torch.equal(si, s_x) and torch.equal(ifl, ifl2) and not ifl.any(), \
        f"{name}: the sealed inverse with an output seal differs from the composition"
    # in place: the timed calls transform what the last call left (the in-place baselines do the same), with no stored seal to hold
    # the moving words against; flags are not read
    calls = (lambda: check(lib.fhe_ntt_forward_sealed(h, P(work), P(work), t._h, ab._h, 1, L, 0, None, P(so), P(fl), sp)),
             lambda: (check(lib.fhe_seal_verify(h, P(work2), P(so2), t._h, 1, L, 0, P(fl2), sp)),
                      check(lib.fhe_ntt_forward_checked(h, P(work2), t._h, ab._h, 1, L, 0, P(fl2[L:]), sp)),
                      check(lib.fhe_seal(h, P(so2), P(work2), t._h, 1, L, 0, sp))),
             lambda: fwd_sealed(dst, x, so, fl), lambda: fwd_composed(dst2, so2, fl2, True), inv_sealed_out, inv_composed)
    reps, out = 10, []
    for r in range(3):
        row = tuple(timed(fn, reps) for fn in calls)
        out.append(row)
        print(f"{name} round {r}: forward sealed in place {row[0]:9.1f} us, verify + checked + seal {row[1]:9.1f} us ({row[0] / row[1]:.3f} x); out of place "
              f"{row[2]:9.1f} us, copy + verify + checked + seal {row[3]:9.1f} us ({row[2] / row[3]:.3f} x); inverse sealed_out {row[4]:9.1f} us, "
              f"inverse_sealed + seal {row[5]:9.1f} us ({row[4] / row[5]:.3f} x)", flush=True)
    summary.append((name, out))
    del t, ab, x, work, work2, dst, dst2, X, iout, iout2
    torch.cuda.empty_cache()
print("summary (round with the median ratio; spread of the ratio over the rounds):")
for name, out in summary:
    for what, base, i, j in (("ntt_forward_sealed in place", "seal_verify + ntt_forward_checked + seal", 0, 1),
                             ("ntt_forward_sealed out of place", "copy + seal_verify + ntt_forward_checked + seal", 2, 3),
                             ("ntt_inverse_sealed_out", "ntt_inverse_sealed + seal", 4, 5)):
        ratio = lambda v: v[i] / v[j]
        m, (lo, hi) = med(out, ratio), spread(out, ratio)
        print(f"  {name}: {what} {m[i]:.1f} us vs {base} {m[j]:.1f} us: {ratio(m):.3f} x ({lo:.3f} .. {hi:.3f})")
