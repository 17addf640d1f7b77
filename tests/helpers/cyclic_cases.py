"""Small and unusual moduli for the cyclic transform (fhe_ntt_cyclic: F.ntt / F.intt / F.four_step_ntt), with the definition they are
held to restated in plain Python integers: the iterative transform of motivation/ntt.py (bit-reverse, then for len = 2, 4 .. n the
butterflies (u + w v, u - w v), w running over powers of root^((mod-1)//len)) and the inverse of motivation/bsgs.py (the same with
root^(mod-2), times n^(mod-2)).  Nothing here imports the library or the emulation.

Where n does not divide mod - 1 the exponent is rounded down and the "transform" is no DFT, and under a composite modulus the
"inverse" inverts nothing; the definition is still a definite function of (a, mod, root), and a case is kept as long as the oracle
and this restatement agree on it (tests/test_cyclic_small_moduli.py: they agree on every case listed, none was dropped)."""
import numpy as np

# (modulus, root, log2 of the lengths)
CASES = [
    (2, 1, (1, 2, 3, 4)), (3, 2, (1, 2, 3, 4)), (17, 3, (1, 2, 3, 4)),
    (257, 3, (5, 8)),
    (65537, 3, (5, 12, 16)),
    (12289, 11, (12,)),
    (1 << 20, 3, (9, 13)),             # even: n never divides mod - 1
    (3 * 65537, 5, (5, 12)),           # odd composite, mod - 1 = 2 * 5 * 19661: rounded exponents from length 4 on
    (998244353, 4, (5, 9)),            # a prime with a root that is no generator: wlen(2) = +1
]
# the roots form one tower (wlen(2) = -1, wlen(2 len)^2 = wlen(len)) at every listed length for these: the natural-order launches serve
# them from 2^5 on, the relabelled forward network serves the rest
TOWER = {(2, 1), (17, 3), (257, 3), (65537, 3), (12289, 11)}


def has_tower(mod: int, root: int, logn: int) -> bool:
    w = [pow(root, (mod - 1) // (2 << s), mod) for s in range(logn)]
    return w[0] == (mod - 1) % mod and all(w[s] * w[s] % mod == w[s - 1] for s in range(1, logn))


def plain_ntt(a, mod: int, root: int):
    n = len(a)
    bits = n.bit_length() - 1
    x = [int(a[int(f"{i:0{bits}b}"[::-1], 2)]) for i in range(n)]
    size = 2
    while size <= n:
        step = pow(root, (mod - 1) // size, mod)
        for start in range(0, n, size):
            w = 1
            for k in range(size // 2):
                lo, hi = x[start + k], x[start + k + size // 2] * w % mod
                x[start + k], x[start + k + size // 2] = (lo + hi) % mod, (lo - hi) % mod
                w = w * step % mod
        size *= 2
    return x


def plain_intt(a, mod: int, root: int):
    scale = pow(len(a), mod - 2, mod)
    return [v * scale % mod for v in plain_ntt(a, mod, pow(root, mod - 2, mod))]


def inputs(mod: int, logn: int):
    """[(name, vector)]: all mod - 1, alternating 0 / mod - 1, all mod // 2, a seeded random vector, and that vector with words at
    and above the modulus (a transform of any word is the transform of its residue)."""
    N = 1 << logn
    rnd = np.random.default_rng(mod % 1000003 + logn).integers(0, mod, N, dtype=np.uint64)
    oor = rnd.copy()
    oor[0], oor[N // 2], oor[N - 1] = 2**64 - 1, mod, mod + mod // 2
    return [("all_qm1", np.full(N, mod - 1, dtype=np.uint64)), ("alt", np.where(np.arange(N) % 2 == 0, 0, mod - 1).astype(np.uint64)),
            ("half", np.full(N, mod // 2, dtype=np.uint64)), ("random", rnd), ("out_of_range", oor)]
