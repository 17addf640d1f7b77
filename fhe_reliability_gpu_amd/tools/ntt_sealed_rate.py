"""Measurement tool: what verifying a key switch's input limbs on the opening transform's own load costs.  Timed with HIP events on
one stream after a warm-up, several rounds alternating in one process at one commit, on resident data.  50-bit ciphertext primes
with 61-bit special primes at BASELINE config 4 (N = 2^17, L = 32, K = 8, dnum = 4) and config 5 (N = 2^16, L = 44, K = 11, dnum =
4); the reference's shape (N = 2^14, six 50-bit primes of which two special: L = 4, K = 2, dnum = 2, plain modulus 65537) in the
BGV form.  Each new call next to the composition it replaces:
  (a) fhe_ntt_inverse_sealed over L rows, out of place, against fhe_seal_verify + a device copy + fhe_ntt_inverse_checked in place;
  (b) fhe_keyswitch_apply_sealed_in against fhe_seal_verify over c's rows + fhe_keyswitch_apply_sealed;
  (c) fhe_rotate_sealed_in against fhe_rotate_sealed_fused, every seal given.
The byte count predicts 32 N against 56 N per row for the transform alone (0.57 x), but the seal kernels have so far run bound by
integer work, not by bytes: the ratios are reported, not promised, and none is a pass condition.
Before timing, the new calls' words, output seals and flags are held against their baselines' on the same operands.
python -m fhe_reliability_gpu_amd.tools.ntt_sealed_rate [--config 4|5|14]"""
import ctypes as C

import torch

import fhe_reliability_gpu_amd as F
from fhe_reliability_gpu_amd._lib import check, lib, vp
from fhe_reliability_gpu_amd.tools import _rate
from fhe_reliability_gpu_amd.tools._rate import med, ptrs, spread

eng = F.Engine(0)
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
P = lambda x: C.c_void_p(x.data_ptr())
h = eng._h
GALOIS = 5


timed = lambda fn, reps: _rate.timed(fn, reps, s)


_rate.print_device()
summary = []
for cfg, logn, L, K, dnum, tp in _rate.configs():
    N, M = 1 << logn, L + K
    qs, t, ks, ab = _rate.plan(eng, logn, L, K, dnum, tp)
    rnd, u64, i32 = _rate.factories(min(qs))
    ops = [rnd(L, N) for _ in range(2)]
    key = rnd(dnum, 2, M, N)                                    # any canonical words time the same
    rows = dnum * 2 * M
    ilay, alay, rlay, flay = ks.apply_sealed_in_layout(), ks.apply_sealed_layout(), ks.rotate_sealed_in_layout(), ks.rotate_sealed_layout()
    assert ilay["fused"], "the plan is above the fused cap: nothing to measure"
    t_dst, t_dst2 = u64(L, N), u64(L, N)
    tflags, tflags2 = i32(2 * L), i32(2 * L)
    iflags, cflags, rflags, rflags2 = i32(ilay["total"]), i32(ilay["total"]), i32(rlay["total"]), i32(flay["total"])
    a_out, c_out, r_out, r_out2 = ([u64(L, N) for _ in range(2)] for _ in range(4))
    r_so, r_so2 = ([u64(L, 2) for _ in range(2)] for _ in range(2))

    seal = lambda words, n_poly, limbs: _rate.seal(eng, t, words, n_poly, limbs, sp)
    s_ops, s_key = [seal(x, 1, L) for x in ops], seal(key, dnum * 2, M)
    sin2 = (vp * 2)(*[x.data_ptr() for x in s_ops])

    intt_sealed = lambda: check(lib.fhe_ntt_inverse_sealed(h, P(t_dst), P(ops[0]), t._h, ab._h, 1, L, 0, P(s_ops[0]), P(tflags), sp))

    def intt_composed():
        check(lib.fhe_seal_verify(h, P(ops[0]), P(s_ops[0]), t._h, 1, L, 0, P(tflags2), sp))
        check(lib.fhe_d2d(h, P(t_dst2), P(ops[0]), L * N * 8, sp))
        check(lib.fhe_ntt_inverse_checked(h, P(t_dst2), t._h, ab._h, 1, L, 0, P(tflags2[L:]), sp))

    apply_in = lambda: check(lib.fhe_keyswitch_apply_sealed_in(h, ks._h, P(a_out[0]), P(a_out[1]), P(ops[0]), P(key), None, None, ab._h, P(s_ops[0]), P(s_key),
                                                               P(iflags), sp))

    def apply_composed():
        check(lib.fhe_seal_verify(h, P(ops[0]), P(s_ops[0]), t._h, 1, L, 0, P(cflags), sp))
        check(lib.fhe_keyswitch_apply_sealed(h, ks._h, P(c_out[0]), P(c_out[1]), P(ops[0]), P(key), None, None, ab._h, P(s_key), P(cflags[L:]), sp))

    def rotate(call, outs, so, fl):
        check(call(h, ks._h, P(outs[0]), P(outs[1]), P(ops[0]), P(ops[1]), GALOIS, P(key), ab._h, sin2, P(s_key), ptrs(so), P(fl), sp))

    rot_in = lambda: rotate(lib.fhe_rotate_sealed_in, r_out, r_so, rflags)
    rot_fused = lambda: rotate(lib.fhe_rotate_sealed_fused, r_out2, r_so2, rflags2)
    name = f"config {cfg}: 2^{logn} L={L} K={K} dnum={dnum}" + (f" t={tp}" if tp else "")
    # the new calls against their baselines on the same operands: words, output seals, flags
    for fn in (intt_sealed, intt_composed, apply_in, apply_composed, rot_in, rot_fused):
        fn()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip([t_dst] + a_out + r_out + r_so, [t_dst2] + c_out + r_out2 + r_so2)), f"{name}: a new call differs from its baseline"
    assert torch.equal(tflags, tflags2) and torch.equal(iflags, cflags), f"{name}: a new call's flags differ"
    assert not tflags.any() and not iflags.any() and not rflags.any() and not rflags2.any(), f"{name}: a clean run raised a flag"
    reps, out = 10, []
    for r in range(3):
        row = (timed(intt_sealed, reps), timed(intt_composed, reps), timed(apply_in, reps), timed(apply_composed, reps), timed(rot_in, reps), timed(rot_fused, reps))
        out.append(row)
        print(f"{name} round {r}: intt sealed {row[0]:9.1f} us, verify + copy + checked {row[1]:9.1f} us ({row[0] / row[1]:.3f} x); apply sealed_in {row[2]:9.1f} us, "
              f"verify(c) + apply_sealed {row[3]:9.1f} us ({row[2] / row[3]:.3f} x); rotate sealed_in {row[4]:9.1f} / sealed_fused {row[5]:9.1f} us "
              f"({row[4] / row[5]:.3f} x)", flush=True)
    torch.cuda.synchronize()
    assert not tflags.any() and not tflags2.any() and not iflags.any() and not cflags.any() and not rflags.any() and not rflags2.any(), f"{name}: a clean run raised a flag"
    summary.append((name, out))
    del ks, ab, ops, key, a_out, c_out, r_out, r_out2
    torch.cuda.empty_cache()
print("summary (round with the median ratio; spread of the ratio over the rounds):")
for name, out in summary:
    for what, base, i, j in (("ntt_inverse_sealed", "seal_verify + copy + ntt_inverse_checked", 0, 1), ("keyswitch_apply_sealed_in", "seal_verify(c) + keyswitch_apply_sealed", 2, 3),
                             ("rotate_sealed_in", "rotate_sealed_fused", 4, 5)):
        ratio = lambda x: x[i] / x[j]
        m, (lo, hi) = med(out, ratio), spread(out, ratio)
        print(f"  {name}: {what} {m[i]:.1f} us vs {base} {m[j]:.1f} us: {ratio(m):.3f} x ({lo:.3f} .. {hi:.3f})")
