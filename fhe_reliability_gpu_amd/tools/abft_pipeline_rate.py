"""Measurement tool: the checked inverse transform against the unchecked one on the headline batch (N = 2^16, 1024
polynomials, 512 MiB), and the checked product against fhe_polymul at the shape of bench.py's polymul_L16x16 leg
(16 distinct 50-bit primes x 16 polynomials); checked and unchecked calls alternate in one process.
python -m fhe_reliability_gpu_amd.tools.abft_pipeline_rate"""
import ctypes as C

import torch

import fhe_reliability_gpu_amd as F
from fhe_reliability_gpu_amd._lib import check, lib

N = 1 << 16
eng = F.Engine(0)
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
P = lambda x: C.c_void_p(x.data_ptr())


def timed(fn, reps, before=None):
    """Mean device time of fn() in microseconds; before() (untimed, same stream) restores inputs that fn consumes."""
    for _ in range(3):
        if before:
            before()
        fn()
    torch.cuda.synchronize()
    total = 0.0
    with torch.cuda.stream(s):
        for _ in range(reps):
            if before:
                before()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            fn()
            b.record(s)
            b.synchronize()
            total += a.elapsed_time(b)
    return total / reps * 1e3


# ---- inverse, 512 MiB batch (one 50-bit prime, 1024 polynomials: bench.py's headline shape)
polys = 1024
q = F.create_moduli(N, [50])
t = eng.tables(16, q)
ab = F.Abft(eng, t)
data = torch.randint(0, q[0], (polys, N), device="cuda", dtype=torch.int64)
flags = torch.zeros(polys * 3, dtype=torch.int32, device="cuda")
plain = lambda: check(lib.fhe_ntt_inverse_batch(eng._h, P(data), t._h, polys, 1, 0, sp))
chk = lambda: check(lib.fhe_ntt_inverse_checked(eng._h, P(data), t._h, ab._h, polys, 1, 0, P(flags), sp))
inv = []
for rnd in range(3):
    u, c = timed(plain, 30), timed(chk, 30)
    inv.append((u, c))
    print(f"inverse 2^16 x 1024 (512 MiB) round {rnd}: unchecked {u:7.1f} us, checked {c:7.1f} us ({c / u:.3f} x)", flush=True)
del data

# ---- product, 16 distinct primes x 16 polynomials (bench.py polymul_L16x16)
L2, P2 = 16, 16
q2 = F.create_moduli(N, [50] * L2)
t2 = eng.tables(16, q2)
ab2 = F.Abft(eng, t2)
mk = lambda: torch.randint(0, q2[0], (P2, L2, N), device="cuda", dtype=torch.int64)
a, b, c = mk(), mk(), mk()
a_keep, b_keep = a.clone(), b.clone()
flags2 = torch.zeros(P2 * L2 * 3, dtype=torch.int32, device="cuda")


def restore():
    a.copy_(a_keep)
    b.copy_(b_keep)


pm = lambda: check(lib.fhe_polymul(eng._h, P(c), P(a), P(b), t2._h, P2, L2, 0, sp))
pmc = lambda: check(lib.fhe_polymul_checked(eng._h, P(c), P(a), P(b), t2._h, ab2._h, P2, L2, 0, P(flags2), sp))
mul = []
for rnd in range(3):
    u, k = timed(pm, 30, restore), timed(pmc, 30, restore)
    mul.append((u, k))
    print(f"polymul 2^16 L16 x 16 round {rnd}: fhe_polymul {u:7.1f} us, checked {k:7.1f} us ({k / u:.3f} x)", flush=True)
torch.cuda.synchronize()
assert not flags.any() and not flags2.any(), "a clean run raised a flag"
mi = sorted(c / u for u, c in inv)[1]
mp = sorted(k / u for u, k in mul)[1]
print(f"summary (median of the rounds): checked inverse {mi:.3f} x unchecked (target <= 1.15), checked product {mp:.3f} x fhe_polymul (target <= 1.30)")
