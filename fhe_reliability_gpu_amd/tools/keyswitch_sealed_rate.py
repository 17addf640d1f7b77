"""Measurement tool: what verifying the switching key on the load that multiplies it costs.  Timed with HIP events on one stream
after a warm-up, several rounds alternating in one process at one commit, on resident data.  50-bit ciphertext primes with 61-bit
special primes at BASELINE config 4 (N = 2^17, L = 32, K = 8, dnum = 4) and config 5 (N = 2^16, L = 44, K = 11, dnum = 4); the
reference's shape (N = 2^14, six 50-bit primes of which two special: L = 4, K = 2, dnum = 2, plain modulus 65537) in the BGV form;
configs 8 and 12 (N = 2^15, K = 2, L = 16 / 24, dnum = 8 / 12) reach the inner product's two widest instantiations.
  (a) fhe_keyswitch_apply_sealed next to the composition it replaces: fhe_seal_verify over the key's rows + fhe_keyswitch_apply_checked;
  (b) fhe_rotate_sealed_fused against fhe_rotate_sealed, every seal given;
  (c) fhe_hmult_sealed_fused_key against fhe_hmult_sealed_fused, rescale on, every seal given;
  (d) stage 3 alone, by difference against fhe_keyswitch_apply_checked in the same round: what the key's sweep costs (composition -
      checked) and what the digests add to the inner product (sealed - checked).
Every fused call reads the key once where its baseline reads it twice: dnum 2 M N 8 bytes fewer per call.  The seal kernels have so
far run bound by integer work, not by bytes, and the fused BSGS inner sum turned out slower than its composition: the ratios are
reported, not promised, and none is a pass condition.
Before timing, the fused calls' words, output seals and flags are held against their baselines' on the same operands.
python -m fhe_reliability_gpu_amd.tools.keyswitch_sealed_rate [--config 4|5|14|8|12]"""
import ctypes as C

import torch

import fhe_reliability_gpu_amd as F
from fhe_reliability_gpu_amd._lib import check, lib
from fhe_reliability_gpu_amd.tools import _rate
from fhe_reliability_gpu_amd.tools._rate import med, ptrs

eng = F.Engine(0)
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
P = lambda x: C.c_void_p(x.data_ptr())
h = eng._h
GALOIS = 5


timed = lambda fn, reps: _rate.timed(fn, reps, s)


_rate.print_device()
summary = []
for cfg, logn, L, K, dnum, tp in _rate.configs(_rate.CONFIGS + ((8, 15, 16, 2, 8, 0), (12, 15, 24, 2, 12, 0))):
    N, M = 1 << logn, L + K
    qs, t, ks, ab = _rate.plan(eng, logn, L, K, dnum, tp)
    rnd, u64, i32 = _rate.factories(min(qs))
    ops = [rnd(L, N) for _ in range(4)]
    key = rnd(dnum, 2, M, N)                                    # any canonical words time the same
    rows = dnum * 2 * M
    alay, rlay, hlay = ks.apply_sealed_layout(), ks.rotate_sealed_layout(), ks.hmult_sealed_layout(True)
    assert alay["fused"], "the plan is above the fused cap: nothing to measure"
    aflags, cflags, rflags, rflags2, hflags, hflags2 = (i32(n) for n in (alay["total"], alay["total"], rlay["total"], rlay["total"], hlay["total"], hlay["total"]))
    a_out, c_out, r_out, r_out2 = ([u64(L, N) for _ in range(2)] for _ in range(4))
    h_out, h_out2 = ([u64(L - 1, N) for _ in range(2)] for _ in range(2))
    r_so, r_so2 = ([u64(L, 2) for _ in range(2)] for _ in range(2))
    h_so, h_so2 = ([u64(L - 1, 2) for _ in range(2)] for _ in range(2))

    seal = lambda words, n_poly, limbs: _rate.seal(eng, t, words, n_poly, limbs, sp)
    s_ops, s_key = [seal(x, 1, L) for x in ops], seal(key, dnum * 2, M)
    sin4, sin2 = ptrs(s_ops), ptrs(s_ops[:2])
    checked_call = lib.fhe_bgv_keyswitch_apply_checked if tp else lib.fhe_keyswitch_apply_checked

    sealed = lambda: check(lib.fhe_keyswitch_apply_sealed(h, ks._h, P(a_out[0]), P(a_out[1]), P(ops[0]), P(key), None, None, ab._h, P(s_key), P(aflags), sp))
    checked = lambda: check(checked_call(h, ks._h, P(c_out[0]), P(c_out[1]), P(ops[0]), P(key), None, None, ab._h, P(cflags[rows:]), sp))

    def composition():
        check(lib.fhe_seal_verify(h, P(key), P(s_key), t._h, dnum * 2, M, 0, P(cflags), sp))
        checked()

    def rotate(call, outs, so, fl):
        check(call(h, ks._h, P(outs[0]), P(outs[1]), P(ops[0]), P(ops[1]), GALOIS, P(key), ab._h, sin2, P(s_key), ptrs(so), P(fl), sp))

    def hmult(call, outs, so, fl):
        check(call(h, ks._h, P(outs[0]), P(outs[1]), *[P(x) for x in ops], P(key), 1, ab._h, sin4, P(s_key), ptrs(so), P(fl), sp))

    rot_fused = lambda: rotate(lib.fhe_rotate_sealed_fused, r_out, r_so, rflags)
    rot_swept = lambda: rotate(lib.fhe_rotate_sealed, r_out2, r_so2, rflags2)
    hm_fused = lambda: hmult(lib.fhe_hmult_sealed_fused_key, h_out, h_so, hflags)
    hm_base = lambda: hmult(lib.fhe_hmult_sealed_fused, h_out2, h_so2, hflags2)
    name = f"config {cfg}: 2^{logn} L={L} K={K} dnum={dnum}" + (f" t={tp}" if tp else "")
    # the fused calls against their baselines on the same operands: words, output seals, flags
    for fn in (sealed, composition, rot_fused, rot_swept, hm_fused, hm_base):
        fn()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a_out + r_out + r_so + h_out + h_so, c_out + r_out2 + r_so2 + h_out2 + h_so2)), f"{name}: a fused call differs from its baseline"
    assert torch.equal(aflags, cflags) and torch.equal(rflags, rflags2) and torch.equal(hflags, hflags2), f"{name}: a fused call's flags differ"
    assert not aflags.any() and not rflags.any() and not hflags.any(), f"{name}: a clean run raised a flag"
    key_mib = rows * N * 8 / 2**20
    reps, out = 10, []
    for r in range(3):
        row = (timed(sealed, reps), timed(composition, reps), timed(checked, reps), timed(rot_fused, reps), timed(rot_swept, reps), timed(hm_fused, reps),
               timed(hm_base, reps))
        out.append(row)
        print(f"{name} round {r}: apply sealed {row[0]:9.1f} us, verify + checked {row[1]:9.1f} us ({row[0] / row[1]:.3f} x), checked alone {row[2]:9.1f} us: the "
              f"sweep costs {row[1] - row[2]:7.1f} us, the digests on the inner product {row[0] - row[2]:7.1f} us; rotate fused {row[3]:9.1f} / swept {row[4]:9.1f} us "
              f"({row[3] / row[4]:.3f} x); hmult fused key {row[5]:9.1f} / fused tensor only {row[6]:9.1f} us ({row[5] / row[6]:.3f} x); key {key_mib:.0f} MiB",
              flush=True)
    torch.cuda.synchronize()
    assert not aflags.any() and not cflags.any() and not rflags.any() and not rflags2.any() and not hflags.any() and not hflags2.any(), f"{name}: a clean run raised a flag"
    summary.append((name, med(out, lambda x: x[0] / x[1]), med(out, lambda x: x[3] / x[4]), med(out, lambda x: x[5] / x[6]), med(out, lambda x: x[0] - x[2])))
    del ks, ab, ops, key, a_out, c_out, r_out, r_out2, h_out, h_out2
    torch.cuda.empty_cache()
print("summary (rounds with the median ratio):")
for name, a, b, c, d in summary:
    print(f"  {name}: apply_sealed {a[0]:.1f} us vs seal_verify(key) + apply_checked {a[1]:.1f} us: {a[0] / a[1]:.3f} x")
    print(f"  {name}: rotate_sealed_fused {b[3]:.1f} us vs rotate_sealed {b[4]:.1f} us: {b[3] / b[4]:.3f} x")
    print(f"  {name}: hmult_sealed_fused_key {c[5]:.1f} us vs hmult_sealed_fused {c[6]:.1f} us: {c[5] / c[6]:.3f} x")
    print(f"  {name}: stage 3 by difference: the key's sweep {d[1] - d[2]:.1f} us, the digests on the inner product {d[0] - d[2]:.1f} us")
