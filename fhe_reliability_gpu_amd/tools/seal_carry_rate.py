"""Measurement tool: what carrying a seal through an add costs.  Timed with HIP events on one stream after a warm-up, several
rounds alternating in one process, on resident data.
  (a) fhe_modadd_sealed over the 2 L rows of a two-part ciphertext at BASELINE config 4 (N = 2^17, L = 32) and config 5 (N = 2^16,
      L = 44), next to fhe_modadd over the same rows and next to the four launch groups it replaces: fhe_seal_verify of each addend,
      fhe_modadd_checked, fhe_seal of the sum.  The carried add moves fhe_modadd's bytes (24 N per row) and the composition twice
      that (48 N), so the byte count predicts at most 1 x fhe_modadd and half the composition; the digest is integer work per word
      and may bound it first on cache-resident rows.  Printed: the times, the ratios, the rate the 24 N bytes imply.  Before timing,
      the carried add's words and seals are held against the composition's on the same operands.
  (b) fhe_rotate_sum_sealed (3 steps) at config 4 (K = 8, dnum = 4) next to the same chain made of fhe_rotate_sealed plus that
      composition per half, CKKS form and BGV form (plain modulus 65537), with the keys' seals.
Reported, not gated.
python -m fhe_reliability_gpu_amd.tools.seal_carry_rate [--skip-rotate]"""
import ctypes as C
import sys

import torch

import fhe_reliability_gpu_amd as F
from fhe_reliability_gpu_amd._lib import check, lib, vp
from fhe_reliability_gpu_amd.tools import _rate
from fhe_reliability_gpu_amd.tools._rate import med

PLAIN_MODULUS = 65537
eng = F.Engine(0)
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
P = lambda x: C.c_void_p(x.data_ptr())
h = eng._h


timed = lambda fn, reps: _rate.timed(fn, reps, s, warmups=3)


def sync():
    check(lib.fhe_sync(h, sp))


_rate.print_device()
summary = []
for cfg, logn, L in ((4, 17, 32), (5, 16, 44)):
    N = 1 << logn
    rows = 2 * L
    qs = F.create_moduli(N, [50] * L)
    t = eng.tables(logn, qs)
    x, y = (torch.randint(0, min(qs), (2, L, N), device="cuda", dtype=torch.int64) for _ in range(2))
    z, z2 = torch.empty_like(x), torch.empty_like(x)
    sx, sy, sz, sz2 = (torch.zeros((rows, 2), device="cuda", dtype=torch.int64) for _ in range(4))
    flags = torch.zeros(4 * rows, device="cuda", dtype=torch.int32)
    fl = [C.c_void_p(flags.data_ptr() + 4 * rows * i) for i in range(4)]
    torch.cuda.synchronize()      # the operands were written on torch's stream, the calls below run on `s`
    check(lib.fhe_seal(h, P(sx), P(x), t._h, 2, L, 0, sp))
    check(lib.fhe_seal(h, P(sy), P(y), t._h, 2, L, 0, sp))
    add = lambda: check(lib.fhe_modadd(h, P(z), P(x), P(y), t._h, 2, L, 0, sp))
    carried = lambda: check(lib.fhe_modadd_sealed(h, P(z), P(x), P(y), P(sz), P(sx), P(sy), None, None, None, t._h, 2, L, 0, fl[0], sp))

    def composed():
        check(lib.fhe_seal_verify(h, P(x), P(sx), t._h, 2, L, 0, fl[1], sp))
        check(lib.fhe_seal_verify(h, P(y), P(sy), t._h, 2, L, 0, fl[2], sp))
        check(lib.fhe_modadd_checked(h, P(z2), P(x), P(y), t._h, 2, L, 0, fl[3], sp))
        check(lib.fhe_seal(h, P(sz2), P(z2), t._h, 2, L, 0, sp))

    carried(), composed(), sync()
    assert torch.equal(z, z2) and torch.equal(sz, sz2) and not flags.any(), "the carried add differs from the composition it replaces"
    out = []
    for rnd in range(5):
        ta, tc, tf = timed(add, 50), timed(carried, 50), timed(composed, 50)
        assert not flags.any(), "a clean run raised a flag"
        out.append((ta, tc, tf))
        print(f"config {cfg} (N = 2^{logn}, {rows} rows) round {rnd}: fhe_modadd {ta:7.1f} us, fhe_modadd_sealed {tc:7.1f} us ({tc / ta:.3f} x), "
              f"verify + verify + modadd_checked + seal {tf:7.1f} us ({tc / tf:.3f} x of it)", flush=True)
    ta, tc, tf = med(out, lambda r: r[1] / r[0])
    nbytes = 3 * rows * N * 8
    summary.append(f"config {cfg}: {nbytes / 2**20:.0f} MiB moved; fhe_modadd {ta:.1f} us ({nbytes / ta / 1e6:.2f} TB/s), fhe_modadd_sealed {tc:.1f} us = "
                   f"{tc / ta:.3f} x ({nbytes / tc / 1e6:.2f} TB/s); the four-launch composition {tf:.1f} us: the carried add takes {tc / tf:.3f} x of it")
    del x, y, z, z2, t

if "--skip-rotate" not in sys.argv:
    logn, L, K, dnum, steps = 17, 32, 8, 4, 3
    N, M = 1 << logn, L + K
    qs, t, ks, ab = _rate.plan(eng, logn, L, K, dnum)
    c_in = [torch.randint(0, min(qs), (L, N), device="cuda", dtype=torch.int64) for _ in range(2)]
    c, w, tmp = ([torch.empty_like(v) for v in c_in] for _ in range(3))
    key = torch.randint(0, min(qs), (dnum, 2, M, N), device="cuda", dtype=torch.int64)      # one key serves every step: the cost is the same
    s_in, s_c, s_w, s_tmp = ([torch.zeros((L, 2), device="cuda", dtype=torch.int64) for _ in range(2)] for _ in range(4))
    skey = torch.zeros((dnum * 2 * M, 2), device="cuda", dtype=torch.int64)
    elts = [pow(3, 1 << i, 2 * N) for i in range(steps)]
    torch.cuda.synchronize()
    for v, sl in zip(c_in, s_in):
        check(lib.fhe_seal(h, P(sl), P(v), t._h, 1, L, 0, sp))
    check(lib.fhe_seal(h, P(skey), P(key), t._h, dnum * 2, M, 0, sp))
    sync()
    a_elts, a_keys, a_skeys = (C.c_uint32 * steps)(*elts), (vp * steps)(*[key.data_ptr()] * steps), (vp * steps)(*[skey.data_ptr()] * steps)
    arr = lambda xs: (vp * 2)(*[v.data_ptr() for v in xs])
    for form, tp in (("CKKS form", 0), ("BGV form", PLAIN_MODULUS)):
        ks.set_plain_modulus(tp)
        lay = ks.rotate_sum_sealed_layout(steps)
        rl = lay["rotate"]["total"]
        flags = torch.zeros(lay["total"] + 8 * L, device="cuda", dtype=torch.int32)
        extra = [C.c_void_p(flags.data_ptr() + 4 * (lay["total"] + L * i)) for i in range(8)]

        def reset(dst, sdst):
            for h_ in range(2):
                dst[h_].copy_(c_in[h_])
                sdst[h_].copy_(s_in[h_])

        def one_call():
            check(lib.fhe_rotate_sum_sealed(h, ks._h, P(c[0]), P(c[1]), P(tmp[0]), P(tmp[1]), steps, a_elts, a_keys, ab._h, arr(s_c), a_skeys, arr(s_tmp),
                                            P(flags), sp))

        def chain():
            for i in range(steps):
                block = C.c_void_p(flags.data_ptr() + 4 * i * lay["stride"])
                check(lib.fhe_rotate_sealed(h, ks._h, P(tmp[0]), P(tmp[1]), P(w[0]), P(w[1]), elts[i], P(key), ab._h, arr(s_w), P(skey), arr(s_tmp), block, sp))
                for h_ in range(2):
                    check(lib.fhe_seal_verify(h, P(w[h_]), P(s_w[h_]), t._h, 1, L, 0, extra[4 * h_], sp))
                    check(lib.fhe_seal_verify(h, P(tmp[h_]), P(s_tmp[h_]), t._h, 1, L, 0, extra[4 * h_ + 1], sp))
                    check(lib.fhe_modadd_checked(h, P(w[h_]), P(w[h_]), P(tmp[h_]), t._h, 1, L, 0, extra[4 * h_ + 2], sp))
                    check(lib.fhe_seal(h, P(s_w[h_]), P(w[h_]), t._h, 1, L, 0, sp))

        # the accumulators grow from call to call; the words stay canonical, so every call does the same work
        with torch.cuda.stream(s):
            reset(c, s_c), reset(w, s_w)
        one_call(), chain(), sync()
        assert all(torch.equal(c[i], w[i]) and torch.equal(s_c[i], s_w[i]) for i in range(2)) and not flags.any(), "the composite differs from the chain it replaces"
        out = []
        for rnd in range(3):
            t1, t2 = timed(one_call, 5), timed(chain, 5)
            assert not flags.any(), "a clean run raised a flag"
            out.append((t1, t2))
            print(f"config 4 {form} round {rnd}: fhe_rotate_sum_sealed ({steps} steps) {t1:9.1f} us, fhe_rotate_sealed + composition {t2:9.1f} us ({t1 / t2:.3f} x)",
                  flush=True)
        t1, t2 = med(out, lambda r: r[0] / r[1])
        summary.append(f"config 4 {form}: fhe_rotate_sum_sealed ({steps} steps, key seals verified) {t1:.1f} us against {t2:.1f} us for fhe_rotate_sealed plus "
                       f"verify + verify + modadd_checked + seal per half: {t1 / t2:.3f} x")
eng.check()
print("summary (median round):")
for line in summary:
    print("  " + line)
