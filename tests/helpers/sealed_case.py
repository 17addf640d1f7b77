"""What the GPU tests of the sealed calls set up in the same way: the plan table, the seeded four-operands-and-one-key case (drawn on
the host, then uploaded and sealed), and the small functions their assertions rest on.  A file whose data has another shape (one
key per step, a list of keys, three parts, diagonals) keeps its own draw and takes the plan construction and the helpers only."""
import numpy as np

P = (1 << 61) - 1
CAP = 12      # digits the fused inner product is instantiated for
# name: (logn, L, K, dnum, limb bits).  A: a row shorter than a chunk; B: a 61-bit prime among 50-bit ones, one chunk per row; C: the
# reference's shape, two chunks per row; D: one digit above the fused cap; E to H: both edges of the fused inner product's two widest
# instantiations (5 to 8 digits, 9 to 12), at the smallest N the checked key switch takes, alpha = 1 and a 61-bit prime among 50-bit
# ones, so that both arithmetic paths run in one launch; I to K: 4, 8 and 16 chunks of 2^13 words per row -- the sealed inner product's
# sweep over more than two chunks and its finish merging 4, 8 and 16 partials -- with a 61-bit prime among 50-bit ones, two and one
# term per digit.  Each file names the subset it runs.
PLANS = {"A": (10, 4, 2, 2, [50] * 6), "B": (13, 3, 1, 3, [50, 61, 50, 50]), "C": (14, 6, 2, 3, [50] * 8), "D": (10, CAP + 1, 1, CAP + 1, [50] * (CAP + 2))}
PLANS.update({name: (5, d, 1, d, [50, 61] + [50] * (d - 1)) for name, d in (("E", 5), ("F", 8), ("G", 9), ("H", 12))})
PLANS.update({"I": (15, 2, 1, 2, [50, 61, 50]), "J": (16, 2, 1, 2, [50, 61, 50]), "K": (17, 2, 1, 1, [50, 61, 50])})
CHUNK = 1 << 13      # words of one chunk of the sealed row sweeps


def plans(names):
    return {n: PLANS[n] for n in names}


class HostCase:
    """the host side of a case, numpy and create_moduli only: ``n_ops`` operands [L][N] drawn limb by limb, then the key
    [dnum][2][L + K][N] digit by half by limb, every word from [margin, q - margin) -- margin 16 keeps a flipped bit 3 below q"""

    def __init__(self, F, plan, seed, margin, n_ops=4):
        self.logn, self.L, self.K, self.dnum, bits = plan
        self.N, self.M = 1 << self.logn, self.L + self.K
        self.qs = F.create_moduli(self.N, bits)
        rng = np.random.default_rng(seed)
        row = lambda q: rng.integers(margin, q - margin, self.N, dtype=np.uint64)
        self.ops = [np.stack([row(q) for q in self.qs[:self.L]]) for _ in range(n_ops)]
        self.key = np.stack([np.stack([np.stack([row(q) for q in self.qs]) for _ in range(2)]) for _ in range(self.dnum)])


class SealedCase(HostCase):
    """a plan's tables, KeySwitch and Abft, and the host case on the device with its seals"""

    def __init__(self, F, eng, plan, seed, margin, n_ops=4):
        super().__init__(F, plan, seed, margin, n_ops)
        self.t = eng.tables(self.logn, self.qs)
        self.ks, self.ab = F.KeySwitch(eng, self.t, self.L, self.K, self.dnum), F.Abft(eng, self.t)
        self.d = [eng.upload(v) for v in self.ops]
        self.dk = eng.upload(self.key)
        self.seals = [self.t.seal(v, limbs=self.L) for v in self.d]
        self.key_seal = self.ks.seal_key(self.dk)

    def unchanged(self):
        return all((dv.download().reshape(-1) == v.reshape(-1)).all() for dv, v in zip(self.d + [self.dk], self.ops + [self.key]))


def sealed_plan(F, eng, plan):
    """(qs, tables, KeySwitch, Abft) of a plan, for the files that draw their own data"""
    logn, L, K, dnum, bits = plan
    qs = F.create_moduli(1 << logn, bits)
    t = eng.tables(logn, qs)
    return qs, t, F.KeySwitch(eng, t, L, K, dnum), F.Abft(eng, t)


def case_cache(make):
    """the body of a module-scoped ``cases`` fixture: get(key) makes a case once and hands the same one out afterwards"""
    made = {}

    def get(key):
        if key not in made:
            made[key] = make(key)
        return made[key]
    return get


class plain_modulus:
    """the BGV form inside the block (t = 0: the CKKS form), the CKKS form again after it"""

    def __init__(self, ks, t):
        self.ks, self.t = ks, t

    def __enter__(self):
        self.ks.set_plain_modulus(self.t)

    def __exit__(self, *exc):
        self.ks.set_plain_modulus(0)


def py_seals(x):
    """[rows][2] Python integers of x = [..., N]: the seal {sum x_j, sum (j + 1) x_j} modulo 2^61 - 1"""
    out = []
    for row in np.asarray(x).reshape(-1, np.shape(x)[-1]).tolist():
        out.append([sum(row) % P, sum((j + 1) * v for j, v in enumerate(row)) % P])
    return out


def py_seals_and_locator(x):
    """[rows][3] Python integers of x = [..., N]: the seal's two sums and the locator sum (j + 1)^2 x_j, which the repairing and the
    carrying calls hold besides -- distinct from py_seals in the third column only"""
    out = []
    for row in np.asarray(x).reshape(-1, np.shape(x)[-1]).tolist():
        out.append([sum(row) % P, sum((j + 1) * v for j, v in enumerate(row)) % P, sum((j + 1) * (j + 1) * v for j, v in enumerate(row)) % P])
    return out


def raised(d, prefix=""):
    """[(name, flat unit)] of every raised word of a (nested) flag dictionary, in the dictionary's order; a None entry is skipped, a
    list of dictionaries is numbered: name[i].inner"""
    out = []
    for name, f in d.items():
        if f is None:
            continue
        if isinstance(f, dict):
            out += raised(f, prefix + name + ".")
        elif isinstance(f, list):
            for i, g in enumerate(f):
                out += raised(g, f"{prefix}{name}[{i}].")
        else:
            out += [(prefix + name, int(u)) for u in np.flatnonzero(np.asarray(f).reshape(-1))]
    return out


def flat(d):
    """[(name, words)] of every flag word of a (nested) flag dictionary, sorted by name at every level; None entries are left out, a
    list of dictionaries is numbered as in raised"""
    out = []
    for name in sorted(d):
        f = d[name]
        if isinstance(f, dict):
            out += [(name + "." + n, v) for n, v in flat(f)]
        elif isinstance(f, list):
            for i, g in enumerate(f):
                out += [(f"{name}[{i}].{n}", v) for n, v in flat(g)]
        elif f is not None:
            out.append((name, np.asarray(f).reshape(-1).tolist()))
    return out


def flip(eng, d, idx, bit):
    """one bit of one word of a device array, flipped in memory"""
    from fhe_reliability_gpu_amd._lib import check, lib
    check(lib.fhe_flip_bit(eng._h, d.ptr, int(idx), int(bit), None))


def same(a, b):
    """two device arrays hold the same words"""
    return (a.download().reshape(-1) == b.download().reshape(-1)).all()


def same_call(x, y):
    """two sealed composites' results (out0, out1, (seal0, seal1), flags): words, output seals and every flag word"""
    return same(x[0], y[0]) and same(x[1], y[1]) and all(same(s, r) for s, r in zip(x[2], y[2])) and flat(x[3]) == flat(y[3])


def safe_coeff(words, q, first, room=16):
    """a coefficient from `first` on whose word stays below q whichever way bit 3 flips (room 64: bits 3 and 4)"""
    return next(j for j in range(first, len(words)) if int(words[j]) < q - room)
