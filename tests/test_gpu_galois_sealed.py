"""The sealed Galois permutation (automorphism_sealed) and the sealed hoisted rotations (rotate_hoisted_sealed) on the GPU: the words
are the unchecked calls', the destination's seal is fhe_seal's, a word wrong at rest raises exactly its row -- for c0 in EVERY
rotation, since every rotation verifies c0 on its own gather --, and a fault on the permutation's own load is seen.

Standalone shapes: log N = 4, 10 and 14 (two chunks per row, so a chunk's source words come from both), rows [2][3] on two 50-bit
primes around a 61-bit one.  Hoisted plans (logn, L, K, dnum): A (10, 4, 2, 2); B (13, 3, 1, 3) with a 61-bit prime; C (14, 6, 2, 3);
D (10, 13, 1, 13), one digit more than the fused inner product is instantiated for: its keys are swept.  Three rotations each.
Words are drawn from [16, q - 16), so that bit-3 flips stay below q.  Corrupted operands are made on the host and uploaded."""
import ctypes as C

import numpy as np
import pytest

from helpers.sealed_case import CAP, case_cache, flat, plans, raised, same, sealed_plan

pytestmark = pytest.mark.gpu

INVALID = 1
SUM, RANGE = 1, 2
WORD, INDEX = 0, 1
PATTERN = 0x5A5A5A5A5A5A5A5A
GRID_CAP = 8192                 # TENSOR_SEAL_GRID_CAP of ntt_launch.hpp: workgroups of the job loop at most
SHAPES = (4, 10, 14)
BITS = [50, 61, 50]
N_POLY, LIMBS = 2, 3
PLANS = plans("ABCD")
N_ROT = 3


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


# ---------------------------------------------------------------------------------------------------------------------------------
# the standalone call
# ---------------------------------------------------------------------------------------------------------------------------------
class Rows:
    """[2][3][N] seeded words on the host and on the device, their seals, and per Galois element the unchecked permutation"""

    def __init__(self, F, eng, logn):
        self.F, self.eng, self.logn, self.N = F, eng, logn, 1 << logn
        self.qs = F.create_moduli(self.N, BITS)
        self.t = eng.tables(logn, self.qs)
        rng = np.random.default_rng(1900 + logn)
        self.src = np.stack([np.stack([rng.integers(16, q - 16, self.N, dtype=np.uint64) for q in self.qs]) for _ in range(N_POLY)])
        self.d = eng.upload(self.src)
        self.seal = self.t.seal(self.d, limbs=LIMBS, n_poly=N_POLY)
        self.ks = (3, 5, 2 * self.N - 1)
        self.ref = {k: F.automorphism(eng, self.t, self.d, k, n_poly=N_POLY, limbs=LIMBS, ntt_domain=True) for k in self.ks}
        self.edge = (1 << 13) if logn > 13 else self.N // 2

    def sealed(self, d, k, **kw):
        return self.F.automorphism_sealed(self.eng, self.t, d, self.seal, k, n_poly=N_POLY, limbs=LIMBS, **kw)

    def changed(self, row, word, value=None, bit=3):
        """a device copy of the rows with one word of flat row `row` changed (default: bit 3 flipped)"""
        bad = self.src.copy().reshape(N_POLY * LIMBS, self.N)
        bad[row, word] = int(bad[row, word]) ^ (1 << bit) if value is None else value
        return self.eng.upload(bad.reshape(self.src.shape))


@pytest.fixture(scope="module")
def rows(F, eng):
    return case_cache(lambda logn: Rows(F, eng, logn))


@pytest.mark.parametrize("logn", SHAPES)
def test_clean_words_are_the_unchecked_calls_and_the_seal_is_fhe_seals(rows, logn):
    c = rows(logn)
    for k in c.ks:
        dst, seal_dst, flags = c.sealed(c.d, k)
        assert same(dst, c.ref[k]), k
        assert same(seal_dst, c.t.seal(dst, limbs=LIMBS, n_poly=N_POLY)), k
        assert flags.shape == (N_POLY * LIMBS,) and not flags.any()
        assert not c.t.seal_verify(dst, seal_dst, limbs=LIMBS, n_poly=N_POLY).any()
        # without a destination seal: the same words and verdict, no seal
        dst2, none, flags2 = c.sealed(c.d, k, seal_out=False)
        assert none is None and same(dst2, dst) and not flags2.any()
    # the destination's seal may be the source's buffer: the finish step reads a row's seal before it writes
    from fhe_reliability_gpu_amd._lib import check, lib
    k = c.ks[1]
    own = c.t.seal(c.d, limbs=LIMBS, n_poly=N_POLY)
    dst, fl = c.eng.alloc(c.src.size), c.eng.upload(np.zeros(4, dtype=np.uint64))
    check(lib.fhe_automorphism_ntt_sealed(c.eng._h, dst.ptr, c.d.ptr, own.ptr, own.ptr, c.t._h, N_POLY, LIMBS, 0, k, fl.ptr, None))
    assert same(own, c.t.seal(c.ref[k], limbs=LIMBS, n_poly=N_POLY)) and not fl.download().any()


@pytest.mark.parametrize("logn", SHAPES)
def test_a_word_wrong_at_rest_raises_its_row_and_poisons_the_destinations_seal(F, rows, logn):
    c = rows(logn)
    for (row, word), k in zip(((0, 0), (N_POLY * LIMBS - 1, c.N - 1), (1, c.edge), (4, c.edge - 1)), (3, 5, 2 * c.N - 1, 5)):
        bad = c.changed(row, word)
        dst, seal_dst, flags = c.sealed(bad, k)
        want = np.zeros(N_POLY * LIMBS, dtype=np.uint32)
        want[row] = SUM
        assert flags.tolist() == want.tolist(), (row, word)
        assert same(dst, F.automorphism(c.eng, c.t, bad, k, n_poly=N_POLY, limbs=LIMBS, ntt_domain=True))      # carries the flipped word
        assert not same(dst, c.ref[k])
        assert c.t.seal_verify(dst, seal_dst, limbs=LIMBS, n_poly=N_POLY).tolist() == want.tolist()      # S0 is the stored one


@pytest.mark.parametrize("logn", SHAPES)
def test_a_word_outside_the_window_raises_range(rows, logn):
    c = rows(logn)
    for row, word, value in ((2, c.N - 1, c.qs[2] + 5), (1, 0, (1 << 64) - 1), (3, c.edge, int(c.src.reshape(-1, c.N)[3, c.edge]) + ((1 << 61) - 1))):
        flags = c.sealed(c.changed(row, word, value=value), 5)[2]
        assert flags[row] & RANGE and np.flatnonzero(flags).tolist() == [row], (row, word)
    # x + p moves no sum: the window alone sees it
    assert flags[3] == RANGE


def test_the_job_loop_takes_a_second_trip(F, eng):
    """cap + 1 rows of two words: the last row is workgroup 0's second job, the one the combine's trailing barrier is for.  At
    N = 2 and k = 3 the slots map 0 -> 1, 1 -> 0 (2 j + 1 times 3 modulo 4): the permutation swaps the two words of a row"""
    P = (1 << 61) - 1
    logn, N, k = 1, 2, 3
    n_poly = GRID_CAP + 1
    qs = F.create_moduli(N, [50])
    t, q = eng.tables(logn, qs), qs[0]
    src = np.random.default_rng(41).integers(16, q - 16, (n_poly, N), dtype=np.uint64)
    assert src.nbytes < 1 << 20
    d = eng.upload(src)
    seal = t.seal(d, limbs=1, n_poly=n_poly)
    dst, seal_dst, flags = F.automorphism_sealed(eng, t, d, seal, k, n_poly=n_poly, limbs=1)
    assert flags.shape == (n_poly,) and not flags.any()
    got, sums = dst.download().reshape(n_poly, N), seal_dst.download().reshape(n_poly, 2)
    assert (got == src[:, ::-1]).all()
    for r in (0, GRID_CAP - 1, GRID_CAP):
        x0, x1 = int(src[r, 1]), int(src[r, 0])
        assert sums[r].tolist() == [(x0 + x1) % P, (x0 + 2 * x1) % P], r
    assert same(seal_dst, t.seal(dst, limbs=1, n_poly=n_poly))
    # a word changed at rest in the last row raises exactly that row
    bad = src.copy()
    bad[GRID_CAP, 1] ^= np.uint64(8)
    flags = F.automorphism_sealed(eng, t, eng.upload(bad), seal, k, n_poly=n_poly, limbs=1)[2]
    assert np.flatnonzero(flags).tolist() == [GRID_CAP] and int(flags[GRID_CAP]) == SUM
    eng.check()


@pytest.mark.parametrize("logn", SHAPES)
def test_the_hook_hits_the_register_and_is_one_shot(rows, logn):
    c = rows(logn)
    k = 5
    for row, coeff, bit in ((0, 0, 63), (5, c.N - 1, 0), (2, c.edge, 33)):
        c.eng.inject_fault_galois_sealed(0, WORD, row, coeff, bit)
        dst, seal_dst, flags = c.sealed(c.d, k)
        assert np.flatnonzero(flags).tolist() == [row] and flags[row] & SUM
        assert (c.d.download().reshape(-1) == c.src.reshape(-1)).all()      # memory stays clean
        diff = np.flatnonzero(dst.download().reshape(-1) != c.ref[k].download().reshape(-1))
        assert diff.tolist() == [row * c.N + coeff]
        assert int(dst.download().reshape(-1)[diff[0]]) ^ int(c.ref[k].download().reshape(-1)[diff[0]]) == 1 << bit
        assert np.flatnonzero(c.t.seal_verify(dst, seal_dst, limbs=LIMBS, n_poly=N_POLY)).tolist() == [row]
        assert not c.sealed(c.d, k)[2].any()      # one shot
    for row, coeff, bit in ((1, 1, 0), (4, c.N - 2, logn - 1)):
        c.eng.inject_fault_galois_sealed(0, INDEX, row, coeff, bit)
        dst, seal_dst, flags = c.sealed(c.d, k)
        assert np.flatnonzero(flags).tolist() == [row] and flags[row] == SUM
        assert np.flatnonzero(dst.download().reshape(-1) != c.ref[k].download().reshape(-1)).tolist() == [row * c.N + coeff]
        assert not c.sealed(c.d, k)[2].any()


@pytest.mark.parametrize("logn", (4, 14))
def test_a_hook_outside_the_call_is_refused_with_nothing_launched(rows, logn):
    from fhe_reliability_gpu_amd._lib import lib
    c = rows(logn)
    rows_n = N_POLY * LIMBS
    for rot, point, row, coeff, bit in ((0, WORD, rows_n, 0, 0), (0, WORD, 0, c.N, 0), (0, INDEX, 0, 0, logn), (1, WORD, 0, 0, 0)):
        c.eng.inject_fault_galois_sealed(rot, point, row, coeff, bit)
        dst = c.eng.upload(np.full(c.src.size, PATTERN, dtype=np.uint64))
        seal_dst = c.eng.upload(np.full(rows_n * 2, PATTERN, dtype=np.uint64))
        fl = c.eng.upload(np.full(rows_n, PATTERN, dtype=np.uint64))
        assert lib.fhe_automorphism_ntt_sealed(c.eng._h, dst.ptr, c.d.ptr, seal_dst.ptr, c.seal.ptr, c.t._h, N_POLY, LIMBS, 0, 5, fl.ptr, None) == INVALID
        c.eng.sync()
        for buf in (dst, seal_dst, fl):
            assert (buf.download() == np.uint64(PATTERN)).all()
        assert not c.sealed(c.d, 5)[2].any()      # the refused call took the hook with it
    # what no call could honour is refused by the setter, and a negative point disarms
    for args in ((0, 2, 0, 0, 0), (-1, WORD, 0, 0, 0), (0, WORD, -1, 0, 0), (0, WORD, 0, -1, 0), (0, WORD, 0, 0, 64)):
        assert lib.fhe_ctx_inject_fault_galois_sealed(c.eng._h, *args) == INVALID
    c.eng.inject_fault_galois_sealed(0, WORD, 0, 0, 5)
    c.eng.inject_fault_galois_sealed(0, -1)
    assert not c.sealed(c.d, 5)[2].any()
    # an even element, an in-place call and a null source seal are refused as well
    dst = c.eng.alloc(c.src.size)
    fl = c.eng.upload(np.full(rows_n, PATTERN, dtype=np.uint64))
    for d_dst, seal_src, k in ((dst, c.seal, 4), (c.d, c.seal, 5), (dst, None, 5)):
        assert lib.fhe_automorphism_ntt_sealed(c.eng._h, d_dst.ptr, c.d.ptr, None, seal_src.ptr if seal_src is not None else None, c.t._h, N_POLY, LIMBS, 0, k,
                                               fl.ptr, None) == INVALID
    assert (fl.download() == np.uint64(PATTERN)).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# the hoisted call
# ---------------------------------------------------------------------------------------------------------------------------------
class Case:
    """a plan, its detector, seeded c0, c1 and three prepared keys on the host and on the device, their seals, and the unchecked and
    the checked hoisted rotations of the clean operands"""

    def __init__(self, F, eng, name):
        self.eng = eng
        self.logn, self.L, self.K, self.dnum, _ = PLANS[name]
        self.N, self.M = 1 << self.logn, self.L + self.K
        self.qs, self.t, self.ks, self.ab = sealed_plan(F, eng, PLANS[name])
        rng = np.random.default_rng(1919 + self.logn + self.dnum)
        poly = lambda: np.stack([rng.integers(16, q - 16, self.N, dtype=np.uint64) for q in self.qs[:self.L]])
        self.c0, self.c1 = poly(), poly()
        self.keys = [np.stack([np.stack([np.stack([rng.integers(16, q - 16, self.N, dtype=np.uint64) for q in self.qs]) for _ in range(2)])
                               for _ in range(self.dnum)]) for _ in range(N_ROT)]
        self.d0, self.d1 = eng.upload(self.c0), eng.upload(self.c1)
        self.dk = [eng.upload(k) for k in self.keys]
        self.seals = (self.t.seal(self.d0, limbs=self.L), self.t.seal(self.d1, limbs=self.L))
        self.key_seals = [self.ks.seal_key(k) for k in self.dk]
        self.elts = [pow(5, i + 1, 2 * self.N) for i in range(N_ROT - 1)] + [2 * self.N - 1]
        self.key_rows = self.dnum * 2 * self.M
        self.fused = self.dnum <= CAP
        self.ref = self.ks.rotate_hoisted(self.d0, self.d1, self.elts, self.dk)
        self.ref_checked = self.ks.rotate_hoisted_checked(self.d0, self.d1, self.elts, self.dk, self.ab)[1]
        self.edge = (1 << 13) if self.logn > 13 else self.N // 2

    def run(self, c0=None, c1=None, keys=None, seals=None, **kw):
        pick = lambda x, own: own if x is None else x
        return self.ks.rotate_hoisted_sealed(pick(c0, self.d0), pick(c1, self.d1), self.elts, pick(keys, self.dk), self.ab, seals=pick(seals, self.seals),
                                             key_seals=self.key_seals, **kw)

    def same_words(self, outs):
        return all(same(o[0], r[0]) and same(o[1], r[1]) for o, r in zip(outs, self.ref))

    def flipped(self, host, row, word, bit=3):
        bad = host.copy().reshape(-1, self.N)
        bad[row, word] = int(bad[row, word]) ^ (1 << bit)
        return self.eng.upload(bad.reshape(host.shape))


@pytest.fixture(scope="module")
def cases(F, eng):
    return case_cache(lambda name: Case(F, eng, name))


@pytest.mark.parametrize("name", list(PLANS))
def test_hoisted_clean_words_flags_and_seals(cases, name):
    c = cases(name)
    lay = c.ks.rotate_hoisted_sealed_layout(N_ROT)
    per = c.L + c.key_rows
    inner = c.ks.rotate_hoisted_checked_layout(N_ROT)["total"]
    assert (lay["c1"], lay["rot0"], lay["rot_words"], lay["checked"], lay["total"], lay["fused"]) == \
        ((0, (c.L,)), c.L, per, c.L + N_ROT * per, c.L + N_ROT * per + inner, c.fused)
    outs, out_seals, fl = c.run()      # the flag buffer starts out as garbage (engine._flag_buffer)
    assert c.same_words(outs)
    assert raised(fl) == []
    assert flat(fl["checked"]) == flat(c.ref_checked)
    assert fl["c1"].shape == (c.L,) and fl["rot_in"][N_ROT - 1]["key"].shape == (c.dnum, 2, c.M) and fl["rot_in"][0]["c0"].shape == (c.L,)
    for o, s in zip(outs, out_seals):
        for h in range(2):
            assert same(s[h], c.t.seal(o[h], limbs=c.L))
    # without any seal: the checked call's words and flags, nothing sealed
    outs, out_seals, fl = c.ks.rotate_hoisted_sealed(c.d0, c.d1, c.elts, c.dk, c.ab, seal_outputs=False)
    assert c.same_words(outs) and raised(fl) == [] and out_seals[0] == (None, None)


@pytest.mark.parametrize("name", list(PLANS))
def test_a_c0_word_wrong_at_rest_raises_its_row_in_every_rotation(cases, name):
    c = cases(name)
    for row, word in ((0, 0), (c.L - 1, c.N - 1), (1, c.edge)):
        outs, _, fl = c.run(c0=c.flipped(c.c0, row, word))
        assert raised(fl) == [(f"rot_in[{r}].c0", row) for r in range(N_ROT)], (row, word)
        assert all(int(fl["rot_in"][r]["c0"][row]) == SUM for r in range(N_ROT))
        assert not c.same_words(outs)


@pytest.mark.parametrize("name", list(PLANS))
def test_a_key_word_raises_its_row_in_its_own_rotation_and_a_c1_word_its_c1_row(cases, name):
    c = cases(name)
    for r, row, word in ((0, 0, 0), (1, c.key_rows - 1, c.N - 1), (2, c.M + 1, c.edge)):
        keys = list(c.dk)
        keys[r] = c.flipped(c.keys[r], row, word)
        outs, _, fl = c.run(keys=keys)
        assert raised(fl) == [(f"rot_in[{r}].key", row)], (r, row, word)
        assert int(fl["rot_in"][r]["key"].reshape(-1)[row]) == SUM
    for row, word in ((0, c.N - 1), (c.L - 1, c.edge - 1)):
        outs, _, fl = c.run(c1=c.flipped(c.c1, row, word))
        assert raised(fl) == [("c1", row)] and int(fl["c1"][row]) == SUM


@pytest.mark.parametrize("name", ["A", "C"])
def test_without_c0s_seal_c0_goes_through_the_checked_permutation(cases, name):
    from fhe_reliability_gpu_amd._lib import check, lib
    c = cases(name)
    outs, _, fl = c.run(seals=(None, c.seals[1]))
    assert c.same_words(outs) and raised(fl) == [] and flat(fl["checked"]) == flat(c.ref_checked)
    # a wrong c0 is then nobody's to see, as in the checked call
    outs, _, fl = c.run(c0=c.flipped(c.c0, 1, 7), seals=(None, c.seals[1]))
    assert raised(fl) == []
    # the checked call's permutation fault on a c0 row (stage 8, unit 2 M + 1): the word the checked call writes
    arm = lambda: check(lib.fhe_ctx_inject_fault_rotate_hoisted(c.eng._h, 1, 8, WORD, 2 * c.M + 1, 9, 30))
    arm()
    want = c.ks.rotate_hoisted_checked(c.d0, c.d1, c.elts, c.dk, c.ab)[1]
    assert raised(want) == [("rot[1].galois", 2 * c.M + 1)]
    arm()
    outs, _, fl = c.run(seals=(None, c.seals[1]))
    assert flat(fl["checked"]) == flat(want) and raised({k: v for k, v in fl.items() if k != "checked"}) == []
    # with c0's seal those rows are the sealed permutation's: the fault has no launch to hit
    arm()
    with pytest.raises(Exception):
        c.run()
    outs, _, fl = c.run()      # the refused call took the hook with it
    assert raised(fl) == [] and c.same_words(outs)


@pytest.mark.parametrize("name", ["A", "C", "D"])
def test_the_hook_hits_one_rotations_gather_and_the_checked_call_leaves_it_armed(cases, name):
    c = cases(name)
    row, coeff, bit = 1, c.edge, 20
    c.eng.inject_fault_galois_sealed(1, WORD, row, coeff, bit)
    outs, _, fl = c.run()
    assert raised(fl) == [("rot_in[1].c0", row)] and int(fl["rot_in"][1]["c0"][row]) == SUM
    assert raised(fl["checked"]) == []
    assert same(outs[0][0], c.ref[0][0]) and same(outs[2][0], c.ref[2][0]) and not same(outs[1][0], c.ref[1][0]) and same(outs[1][1], c.ref[1][1])
    assert (c.d0.download().reshape(-1) == c.c0.reshape(-1)).all()
    assert raised(c.run()[2]) == []      # one shot
    # the checked call does not run the step: it leaves the hook armed and sees nothing
    c.eng.inject_fault_galois_sealed(1, INDEX, row, coeff, 0)
    outs, cf = c.ks.rotate_hoisted_checked(c.d0, c.d1, c.elts, c.dk, c.ab)
    assert raised(cf) == [] and c.same_words(outs)
    assert raised(c.run()[2]) == [("rot_in[1].c0", row)]
    # outside the call: a rotation, a row, a word, an index bit that do not exist; a null c0 seal
    for args in ((N_ROT, WORD, 0, 0, 0), (0, WORD, c.L, 0, 0), (0, WORD, 0, c.N, 0), (0, INDEX, 0, 0, c.logn)):
        c.eng.inject_fault_galois_sealed(*args)
        with pytest.raises(Exception):
            c.run()
        assert raised(c.run()[2]) == []
    c.eng.inject_fault_galois_sealed(0, WORD, 0, 0, 0)
    with pytest.raises(Exception):
        c.run(seals=(None, c.seals[1]))
    assert raised(c.run()[2]) == []
