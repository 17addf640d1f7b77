"""Measurement tool: the residue-checked element-wise products against the unchecked ones, checked and unchecked calls
alternating in one process -- fhe_modmul and fhe_modmul_acc at the shape of bench.py's modmul_L16x16 leg (16 distinct 50-bit
primes x 16 polynomials of 2^16), and fhe_tensor_product at BASELINE config 4's shape (N = 2^17, L = 32).
python -m fhe_reliability_gpu_amd.tools.pointwise_check_rate"""
import ctypes as C

import torch

import fhe_reliability_gpu_amd as F
from fhe_reliability_gpu_amd._lib import check, lib
from fhe_reliability_gpu_amd.tools import _rate

eng = F.Engine(0)
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
P = lambda x: C.c_void_p(x.data_ptr())


timed = lambda fn, reps: _rate.timed(fn, reps, s, warmups=3)


def compare(name, plain, checked, flags, reps=50, rounds=3):
    out = []
    for rnd in range(rounds):
        u, c = timed(plain, reps), timed(checked, reps)
        out.append((u, c))
        print(f"{name} round {rnd}: unchecked {u:7.1f} us, checked {c:7.1f} us ({c / u:.3f} x)", flush=True)
    torch.cuda.synchronize()
    assert not flags.any(), f"{name}: a clean run raised a flag"
    return sorted(c / u for u, c in out)[rounds // 2]


# ---- modmul / modmul-acc, 16 distinct 50-bit primes x 16 polynomials of 2^16 (bench.py modmul_L16x16)
N, L, PL = 1 << 16, 16, 16
qs = F.create_moduli(N, [50] * L)
t = eng.tables(16, qs)
mk = lambda: torch.randint(0, min(qs), (PL, L, N), device="cuda", dtype=torch.int64)
a, b, c = mk(), mk(), mk()
flags = torch.zeros(PL * L, dtype=torch.int32, device="cuda")
mm = compare("modmul 2^16 L16 x 16",
             lambda: check(lib.fhe_modmul(eng._h, P(c), P(a), P(b), t._h, PL, L, 0, sp)),
             lambda: check(lib.fhe_modmul_checked(eng._h, P(c), P(a), P(b), t._h, PL, L, 0, P(flags), sp)), flags)
# accumulating into c: it stays canonical, so every call is a clean checked call
ma = compare("modmul_acc 2^16 L16 x 16",
             lambda: check(lib.fhe_modmul_acc(eng._h, P(c), P(a), P(b), t._h, PL, L, 0, sp)),
             lambda: check(lib.fhe_modmul_acc_checked(eng._h, P(c), P(a), P(b), t._h, PL, L, 0, P(flags), sp)), flags)
del a, b, c

# ---- tensor product, N = 2^17, L = 32 (both arithmetic paths: 24 limbs of 50 bits on FP64, 8 of 61 bits on U64)
N2, L2 = 1 << 17, 32
q2 = F.create_moduli(N2, [50 if i % 4 else 61 for i in range(L2)])
t2 = eng.tables(17, q2)
mk2 = lambda: torch.randint(0, min(q2), (L2, N2), device="cuda", dtype=torch.int64)
a0, a1, b0, b1, d0, d1, d2 = (mk2() for _ in range(7))
flags2 = torch.zeros(3 * L2, dtype=torch.int32, device="cuda")
tp = compare("tensor 2^17 L32",
             lambda: check(lib.fhe_tensor_product(eng._h, P(d0), P(d1), P(d2), P(a0), P(a1), P(b0), P(b1), t2._h, L2, 0, sp)),
             lambda: check(lib.fhe_tensor_product_checked(eng._h, P(d0), P(d1), P(d2), P(a0), P(a1), P(b0), P(b1), t2._h, L2, 0, P(flags2), sp)),
             flags2)
verdict = lambda r, lim: f"target <= {lim:.2f}: {'met' if r <= lim else 'missed'}"
print(f"summary (median of the rounds): modmul {mm:.3f} x ({verdict(mm, 1.10)}), modmul_acc {ma:.3f} x ({verdict(ma, 1.10)}), "
      f"tensor {tp:.3f} x ({verdict(tp, 1.15)})")
