"""Measurement tool: what verifying a permutation's source on its own gather costs.  Timed with HIP events on one stream after a
warm-up, several rounds alternating in one process at one commit, on resident data.  50-bit ciphertext primes with 61-bit special
primes at BASELINE config 4 (N = 2^17, L = 32, K = 8, dnum = 4) and config 5 (N = 2^16, L = 44, K = 11, dnum = 4).
  (a) fhe_automorphism_ntt_sealed over the 2 L rows of a ciphertext next to the composition it replaces: fhe_seal_verify +
      fhe_automorphism_ntt_checked + fhe_seal over the same rows; and without a destination seal against the first two;
  (b) fhe_rotate_hoisted_sealed at 8 rotations, every seal given, next to the composition: sweeps of c0, c1 and the 8 prepared keys,
      fhe_rotate_hoisted_checked, 16 output sweeps.
The sealed permutation moves 16 N bytes per row where the composition moves 40 N (0.4); the hoisted call reads every key and c0
once fewer (and gathers c0 through the sealed kernel 8 times where the checked one gathered it 8 times and read it linearly 8 times
more).  The seal kernels have so far run bound by integer work, not by bytes: the ratios are reported, not promised, and none is a
pass condition.  Before timing, words, seals and flags are held against the composition's on the same operands.
python -m fhe_reliability_gpu_amd.tools.galois_sealed_rate [--config 4|5]"""
import ctypes as C

import torch

import fhe_reliability_gpu_amd as F
from fhe_reliability_gpu_amd._lib import check, lib, vp
from fhe_reliability_gpu_amd.tools import _rate
from fhe_reliability_gpu_amd.tools._rate import ptrs

eng = F.Engine(0)
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
P = lambda x: C.c_void_p(x.data_ptr())
h = eng._h
GALOIS = 5
N_ROT = 8


timed = lambda fn, reps: _rate.timed(fn, reps, s)


def spread(rows, key):
    v = sorted(key(r) for r in rows)
    return v[len(v) // 2], v[0], v[-1]


_rate.print_device()
summary = []
for cfg, logn, L, K, dnum in _rate.configs(((4, 17, 32, 8, 4), (5, 16, 44, 11, 4))):
    N, M = 1 << logn, L + K
    qs, t, ks, ab = _rate.plan(eng, logn, L, K, dnum)
    rnd, u64, i32 = _rate.factories(min(qs))

    seal = lambda words, n_poly, limbs: _rate.seal(eng, t, words, n_poly, limbs, sp)
    # ---- (a) the permutation over the 2 L rows of a ciphertext
    ct = rnd(2, L, N)
    s_ct = seal(ct, 2, L)
    dst_s, dst_n, dst_c = u64(2, L, N), u64(2, L, N), u64(2, L, N)
    sd_s, sd_c = u64(2 * L, 2), u64(2 * L, 2)
    f_s, f_n, f_v, f_c = i32(2 * L), i32(2 * L), i32(2 * L), i32(2 * L)
    perm_sealed = lambda: check(lib.fhe_automorphism_ntt_sealed(h, P(dst_s), P(ct), P(sd_s), P(s_ct), t._h, 2, L, 0, GALOIS, P(f_s), sp))
    perm_noseal = lambda: check(lib.fhe_automorphism_ntt_sealed(h, P(dst_n), P(ct), None, P(s_ct), t._h, 2, L, 0, GALOIS, P(f_n), sp))

    def perm_front():
        check(lib.fhe_seal_verify(h, P(ct), P(s_ct), t._h, 2, L, 0, P(f_v), sp))
        check(lib.fhe_automorphism_ntt_checked(h, P(dst_c), P(ct), logn, GALOIS, 2 * L, P(f_c), sp))

    def perm_comp():
        perm_front()
        check(lib.fhe_seal(h, P(sd_c), P(dst_c), t._h, 2, L, 0, sp))

    # ---- (b) the hoisted rotations
    c0, c1 = rnd(L, N), rnd(L, N)
    keys = [rnd(dnum, 2, M, N) for _ in range(N_ROT)]      # any canonical words time the same
    s_c0, s_c1, s_keys = seal(c0, 1, L), seal(c1, 1, L), [seal(k, dnum * 2, M) for k in keys]
    elts = (C.c_uint32 * N_ROT)(*[pow(5, i + 1, 2 * N) for i in range(N_ROT)])
    lay, clay = ks.rotate_hoisted_sealed_layout(N_ROT), ks.rotate_hoisted_checked_layout(N_ROT)
    outs_s, outs_c = ([[u64(L, N) for _ in range(N_ROT)] for _ in range(2)] for _ in range(2))
    so_s, so_c = ([[u64(L, 2) for _ in range(N_ROT)] for _ in range(2)] for _ in range(2))
    hf_s, hf_c, hf_in = i32(lay["total"]), i32(clay["total"]), i32(lay["checked"])
    sin = (vp * 2)(s_c0.data_ptr(), s_c1.data_ptr())
    hoisted_sealed = lambda: check(lib.fhe_rotate_hoisted_sealed(h, ks._h, ptrs(outs_s[0]), ptrs(outs_s[1]), P(c0), P(c1), elts, ptrs(keys), N_ROT, ab._h, sin,
                                                                ptrs(s_keys), ptrs(so_s[0]), ptrs(so_s[1]), P(hf_s), sp))
    hoisted_checked = lambda: check(lib.fhe_rotate_hoisted_checked(h, ks._h, ptrs(outs_c[0]), ptrs(outs_c[1]), P(c0), P(c1), elts, ptrs(keys), N_ROT, ab._h,
                                                                  P(hf_c), sp))
    per = lay["rot_words"]

    def hoisted_comp():
        check(lib.fhe_seal_verify(h, P(c1), P(s_c1), t._h, 1, L, 0, P(hf_in), sp))
        for r in range(N_ROT):      # c0 once (into rotation 0's words), every key
            if r == 0:
                check(lib.fhe_seal_verify(h, P(c0), P(s_c0), t._h, 1, L, 0, P(hf_in[L:]), sp))
            check(lib.fhe_seal_verify(h, P(keys[r]), P(s_keys[r]), t._h, dnum * 2, M, 0, P(hf_in[L + r * per + L:]), sp))
        hoisted_checked()
        for r in range(N_ROT):
            for half in range(2):
                check(lib.fhe_seal(h, P(so_c[half][r]), P(outs_c[half][r]), t._h, 1, L, 0, sp))

    name = f"config {cfg}: 2^{logn} L={L} K={K} dnum={dnum}"
    for fn in (perm_sealed, perm_noseal, perm_comp, hoisted_sealed, hoisted_comp):
        fn()
    torch.cuda.synchronize()
    assert torch.equal(dst_s, dst_c) and torch.equal(dst_n, dst_c) and torch.equal(sd_s, sd_c), f"{name}: the sealed permutation differs from the composition"
    assert all(torch.equal(x, y) for a, b in zip(outs_s + so_s, outs_c + so_c) for x, y in zip(a, b)), f"{name}: the sealed hoisted call differs from the composition"
    assert torch.equal(hf_s[lay["checked"]:], hf_c), f"{name}: the checked block differs"
    assert not any(x.any() for x in (f_s, f_n, f_v, f_c, hf_s, hf_c, hf_in)), f"{name}: a clean run raised a flag"
    reps, out = 10, []
    for r in range(3):
        row = (timed(perm_sealed, reps), timed(perm_comp, reps), timed(perm_noseal, reps), timed(perm_front, reps), timed(hoisted_sealed, 3), timed(hoisted_comp, 3),
               timed(hoisted_checked, 3))
        out.append(row)
        print(f"{name} round {r}: permutation sealed {row[0]:8.1f} us, verify + checked + seal {row[1]:8.1f} us ({row[0] / row[1]:.3f} x); without a destination "
              f"seal {row[2]:8.1f} us, verify + checked {row[3]:8.1f} us ({row[2] / row[3]:.3f} x); hoisted x{N_ROT} sealed {row[4]:9.1f} us, composition "
              f"{row[5]:9.1f} us ({row[4] / row[5]:.3f} x), checked alone {row[6]:9.1f} us", flush=True)
    torch.cuda.synchronize()
    assert not any(x.any() for x in (f_s, f_n, f_v, f_c, hf_s, hf_c, hf_in)), f"{name}: a clean run raised a flag"
    summary.append((name, out))
    del ks, ab, keys, outs_s, outs_c, ct, dst_s, dst_n, dst_c
    torch.cuda.empty_cache()
print("summary (median ratio over the rounds [lowest, highest]; times of the median round):")
for name, out in summary:
    for label, a, b in (("automorphism_ntt_sealed vs seal_verify + automorphism_ntt_checked + seal", 0, 1),
                        ("automorphism_ntt_sealed without a destination seal vs seal_verify + automorphism_ntt_checked", 2, 3),
                        (f"rotate_hoisted_sealed x{N_ROT} vs sweeps + rotate_hoisted_checked + output sweeps", 4, 5),
                        (f"rotate_hoisted_sealed x{N_ROT} vs rotate_hoisted_checked alone", 4, 6)):
        m, lo, hi = spread(out, lambda x: x[a] / x[b])
        mid = sorted(out, key=lambda x: x[a] / x[b])[len(out) // 2]
        print(f"  {name}: {label}: {mid[a]:.1f} vs {mid[b]:.1f} us: {m:.3f} x [{lo:.3f}, {hi:.3f}]")
