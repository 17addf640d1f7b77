"""Measurement tool: what verifying a rescale's input on the loads that consume it, and sealing a call's outputs from the registers
its last launch stores, costs.  Timed with HIP events on one stream after a warm-up, several rounds alternating in one process at
one commit, on resident data.  50-bit ciphertext primes with 61-bit special primes at BASELINE config 4 (N = 2^17, L = 32, K = 8,
dnum = 4) and config 5 (N = 2^16, L = 44, K = 11, dnum = 4); the reference's shape (N = 2^14, six 50-bit primes of which two
special: L = 4, K = 2, dnum = 2, plain modulus 65537) in the BGV form.  Each new call next to what it replaces:
  (a) fhe_rescale_sealed over two parts against fhe_seal_verify + the checked rescale of the plan's form + fhe_seal;
  (b) fhe_hmult_sealed_out against fhe_hmult_sealed_fused_key, with rescale, every seal given;
  (c) fhe_rotate_sealed_out against fhe_rotate_sealed_in, every seal given.
The byte count says (a) saves one read of the 2 L input rows, one of the 2 (L - 1) output rows and the last limbs' copy, (b) and
(c) one read of 2 (L - 1) or 2 L rows; the seal kernels have so far run bound by integer work, not by bytes: the ratios are
reported, not promised, and none is a pass condition.
Before timing, the new calls' words, output seals and flags are held against their baselines' on the same operands.
python -m fhe_reliability_gpu_amd.tools.subscale_sealed_rate [--config 4|5|14]"""
import ctypes as C

import torch

import fhe_reliability_gpu_amd as F
from fhe_reliability_gpu_amd._lib import check, lib
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
    N, M, R = 1 << logn, L + K, L - 1
    qs, t, ks, ab = _rate.plan(eng, logn, L, K, dnum, tp)
    rnd, u64, i32 = _rate.factories(min(qs))
    ops = [rnd(L, N) for _ in range(4)]
    ct = rnd(2, L, N)
    key = rnd(dnum, 2, M, N)                                    # any canonical words time the same
    slay, hlay, rlay = ks.rescale_sealed_layout(2), ks.hmult_sealed_layout(True), ks.rotate_sealed_in_layout()
    rescale_checked = lib.fhe_bgv_mod_switch_checked if tp else lib.fhe_rescale_checked

    seal = lambda words, n_poly, limbs: _rate.seal(eng, t, words, n_poly, limbs, sp)
    s_ops, s_ct, s_key = [seal(x, 1, L) for x in ops], seal(ct, 2, L), seal(key, dnum * 2, M)
    sin4, sin2 = ptrs(s_ops), ptrs(s_ops[:2])
    rs_out, rs_out2, rs_so, rs_so2 = u64(2, R, N), u64(2, R, N), u64(2 * R, 2), u64(2 * R, 2)
    rs_fl, rs_fl2 = i32(slay["total"]), i32(slay["total"])
    hm_out, hm_out2, hm_so, hm_so2 = ([u64(R, N) for _ in range(2)], [u64(R, N) for _ in range(2)], [u64(R, 2) for _ in range(2)], [u64(R, 2) for _ in range(2)])
    hm_fl, hm_fl2 = i32(hlay["total"]), i32(hlay["total"])
    ro_out, ro_out2, ro_so, ro_so2 = ([u64(L, N) for _ in range(2)], [u64(L, N) for _ in range(2)], [u64(L, 2) for _ in range(2)], [u64(L, 2) for _ in range(2)])
    ro_fl, ro_fl2 = i32(rlay["total"]), i32(rlay["total"])

    rescale_sealed = lambda: check(lib.fhe_rescale_sealed(h, ks._h, P(rs_out), P(ct), 2, ab._h, P(s_ct), P(rs_so), P(rs_fl), sp))

    def rescale_composed():
        check(lib.fhe_seal_verify(h, P(ct), P(s_ct), t._h, 2, L, 0, P(rs_fl2), sp))
        check(rescale_checked(h, ks._h, P(rs_out2), P(ct), 2, ab._h, P(rs_fl2[2 * L:]), sp))
        check(lib.fhe_seal(h, P(rs_so2), P(rs_out2), t._h, 2, R, 0, sp))

    def hmult(call, outs, so, fl):
        check(call(h, ks._h, P(outs[0]), P(outs[1]), P(ops[0]), P(ops[1]), P(ops[2]), P(ops[3]), P(key), 1, ab._h, sin4, P(s_key), ptrs(so), P(fl), sp))

    def rotate(call, outs, so, fl):
        check(call(h, ks._h, P(outs[0]), P(outs[1]), P(ops[0]), P(ops[1]), GALOIS, P(key), ab._h, sin2, P(s_key), ptrs(so), P(fl), sp))

    hm_new, hm_old = lambda: hmult(lib.fhe_hmult_sealed_out, hm_out, hm_so, hm_fl), lambda: hmult(lib.fhe_hmult_sealed_fused_key, hm_out2, hm_so2, hm_fl2)
    ro_new, ro_old = lambda: rotate(lib.fhe_rotate_sealed_out, ro_out, ro_so, ro_fl), lambda: rotate(lib.fhe_rotate_sealed_in, ro_out2, ro_so2, ro_fl2)
    fns = (rescale_sealed, rescale_composed, hm_new, hm_old, ro_new, ro_old)
    name = f"config {cfg}: 2^{logn} L={L} K={K} dnum={dnum}" + (f" t={tp}" if tp else "")
    # the new calls against their baselines on the same operands: words, output seals, flags
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    new, old = [rs_out, rs_so] + hm_out + hm_so + ro_out + ro_so, [rs_out2, rs_so2] + hm_out2 + hm_so2 + ro_out2 + ro_so2
    assert all(torch.equal(x, y) for x, y in zip(new, old)), f"{name}: a new call differs from its baseline"
    assert torch.equal(rs_fl, rs_fl2) and torch.equal(hm_fl, hm_fl2) and torch.equal(ro_fl, ro_fl2), f"{name}: a new call's flags differ"
    assert not rs_fl.any() and not hm_fl.any() and not ro_fl.any(), f"{name}: a clean run raised a flag"
    reps, out = 10, []
    for r in range(3):
        row = tuple(timed(fn, reps) for fn in fns)
        out.append(row)
        print(f"{name} round {r}: rescale sealed {row[0]:9.1f} us, verify + checked + seal {row[1]:9.1f} us ({row[0] / row[1]:.3f} x); hmult sealed_out {row[2]:9.1f} / "
              f"sealed_fused_key {row[3]:9.1f} us ({row[2] / row[3]:.3f} x); rotate sealed_out {row[4]:9.1f} / sealed_in {row[5]:9.1f} us ({row[4] / row[5]:.3f} x)",
              flush=True)
    torch.cuda.synchronize()
    assert not any(f.any() for f in (rs_fl, rs_fl2, hm_fl, hm_fl2, ro_fl, ro_fl2)), f"{name}: a clean run raised a flag"
    summary.append((name, out))
    del ks, ab, ops, ct, key, new, old
    torch.cuda.empty_cache()
print("summary (round with the median ratio; spread of the ratio over the rounds):")
for name, out in summary:
    for what, base, i, j in (("rescale_sealed", "seal_verify + checked rescale + seal", 0, 1), ("hmult_sealed_out", "hmult_sealed_fused_key", 2, 3),
                             ("rotate_sealed_out", "rotate_sealed_in", 4, 5)):
        ratio = lambda x: x[i] / x[j]
        m, (lo, hi) = med(out, ratio), spread(out, ratio)
        print(f"  {name}: {what} {m[i]:.1f} us vs {base} {m[j]:.1f} us: {ratio(m):.3f} x ({lo:.3f} .. {hi:.3f})")
