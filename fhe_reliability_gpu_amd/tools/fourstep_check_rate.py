"""Measurement tool: the ABFT-checked four-step transform against the unchecked one, the calls alternating in one process --
fhe_fourstep_ntt_batch, fhe_fourstep_ntt_checked and fhe_fourstep_ntt_checked_phases on 256 vectors of 2^16 (128 MiB, stays in
the Infinity Cache) and on 1024 vectors (512 MiB, streams from HBM and runs as sub-batches), for 998244353 (FP64 path) and for a
61-bit prime (integer path).  The yardstick is the unchecked call of the same process, never a number from another run.
python -m fhe_reliability_gpu_amd.tools.fourstep_check_rate"""
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


def shape(name, mod, g, n_vec, reps=20, rounds=3):
    N = 1 << 16
    fs = F.FourStep(eng, 256, 256, mod, g)
    fs.prepare_checked()
    src = torch.randint(0, mod, (n_vec, N), device="cuda", dtype=torch.int64)
    dst = torch.empty_like(src)
    flags = torch.zeros(3 * n_vec, dtype=torch.int32, device="cuda")
    plain = lambda: check(lib.fhe_fourstep_ntt_batch(eng._h, P(dst), P(src), fs._h, n_vec, sp))
    whole = lambda: check(lib.fhe_fourstep_ntt_checked(eng._h, P(dst), P(src), fs._h, n_vec, P(flags), sp))
    phases = lambda: check(lib.fhe_fourstep_ntt_checked_phases(eng._h, P(dst), P(src), fs._h, n_vec, P(flags), sp))
    out = []
    for rnd in range(rounds):
        u, w, p = timed(plain, reps), timed(whole, reps), timed(phases, reps)
        out.append((w / u, p / u))
        print(f"{name} round {rnd}: unchecked {u:8.1f} us, checked {w:8.1f} us ({w / u:.3f} x), per-phase {p:8.1f} us ({p / u:.3f} x)", flush=True)
    torch.cuda.synchronize()
    assert not flags.any(), f"{name}: a clean run raised a flag"
    fs.close()
    med = lambda k: sorted(r[k] for r in out)[rounds // 2]
    return med(0), med(1)


q61 = F.create_moduli(1 << 16, [61])[0]
g61 = next(c for c in range(2, 1000) if pow(c, (q61 - 1) // 2, q61) == q61 - 1)
for label, mod, g in (("998244353", 998244353, 3), ("61-bit", q61, g61)):
    for n_vec in (256, 1024):
        w, p = shape(f"2^16 x {n_vec} mod {label}", mod, g, n_vec)
        print(f"summary (median of the rounds) 2^16 x {n_vec} mod {label}: checked {w:.3f} x, per-phase {p:.3f} x of the unchecked call")
