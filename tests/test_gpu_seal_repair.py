"""The seal repair on the GPU: the locator sum, fhe_seal_repair and the repairing multiply / rotation.  Sums are held against Python
integers computed here from the host arrays; corruption is made in device memory with fhe_flip_bit.

Primitives: N = 2^5 (a row below one chunk, idle lanes), 2^13 (exactly one chunk), 2^14 (two chunks) as two polynomials of three
limbs from table limb 1 on (61, 50, 61 bits), and N = 2^17 as three limbs (50, 61, 50), where (j + 1)^2 passes 2^32.  Every row
carries the words the two-word traps need: bit 7 clear in words 2, 4 and 10, bit 8 set in word 9, and word 20 = word 5 ^ 0b101.

Composites: the 2^13 plan (L 3, K 1, dnum 3, mixed 50 / 61-bit limbs) in the CKKS and the BGV form."""
import ctypes as C

import numpy as np
import pytest

from helpers.checked_plan import limb_bits
from helpers.sealed_case import P, SealedCase, case_cache, flip, plain_modulus, py_seals_and_locator, raised, safe_coeff

pytestmark = pytest.mark.gpu

INVALID = 1
SUM, RANGE = 1, 2
CLEAN, REPAIRED, UNCORRECTABLE, TRANSIENT, SUSPECT = 0, 1, 2, 3, 4
GARBAGE = 0x5A5A5A5A5A5A5A5A
SHAPES = {5: (2, 3, 1), 13: (2, 3, 1), 14: (2, 3, 1), 17: (1, 3, 0)}      # logn: (n_poly, limbs, start_idx)


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


class Rows:
    """rows of one size on the device with their seals and locators, and the reference sums, computed once"""

    def __init__(self, F, eng, logn):
        self.logn, self.N = logn, 1 << logn
        self.n_poly, self.limbs, self.start = SHAPES[logn]
        N = self.N
        self.qs = F.create_moduli(N, [50, 61, 50] if logn == 17 else limb_bits("mixed", 5, 2))      # 50 61 50 61 50 | 61 50
        self.t = eng.tables(logn, self.qs)
        self.rows = self.n_poly * self.limbs
        self.q_of = [self.qs[self.start + r % self.limbs] for r in range(self.rows)]
        rng = np.random.default_rng(logn)
        x = np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in self.q_of])
        self.mid = 1 << 13 if logn > 13 else N // 2      # either side of the chunk boundary where there is one
        self.spots = [0, self.mid, N - 1]
        x[:, self.spots] = (x[:, self.spots] >> np.uint64(1)) | np.uint64(1)      # odd and below q / 2: x + p is bits 0 and 61
        x[:, [2, 4, 10]] &= ~np.uint64(1 << 7)
        x[:, 9] = (x[:, 9] >> np.uint64(1)) | np.uint64(1 << 8)
        x[:, 5] >>= np.uint64(1)
        x[:, 20] = x[:, 5] ^ np.uint64(0b101)
        assert all((x[r] < np.uint64(q)).all() for r, q in enumerate(self.q_of))
        self.x = x
        self.kw = dict(limbs=self.limbs, start=self.start, n_poly=self.n_poly)
        self.d = eng.upload(x)
        self.want = py_seals_and_locator(x)
        self.seal = self.t.seal(self.d, **self.kw)
        self.loc = self.t.seal_locator(self.d, **self.kw)

    def repair(self):
        return self.t.seal_repair(self.d, self.seal, self.loc, **self.kw)

    def only(self, rows, value, width=None):
        rows = {r: value for r in rows} if not isinstance(rows, dict) else rows
        zero = 0 if width is None else [0] * width
        return [rows.get(r, zero) for r in range(self.rows)]


@pytest.fixture(scope="module")
def rows_of(F, eng):
    return case_cache(lambda logn: Rows(F, eng, logn))


LOGNS = [5, 13, 14, 17]


@pytest.mark.parametrize("logn", LOGNS)
def test_the_locator_equals_the_python_sum_and_a_clean_call_touches_nothing(eng, rows_of, logn):
    c = rows_of(logn)
    assert c.seal.download().tolist() == [w[:2] for w in c.want]
    got = c.loc.download()
    assert got.tolist() == [w[2] for w in c.want]
    # reruns into other buffers: identical, bit for bit
    assert all(c.t.seal_locator(c.d, **c.kw).download().tobytes() == got.tobytes() for _ in range(3))
    flags, report = c.repair()
    assert flags.tolist() == [0] * c.rows and report.tolist() == [[CLEAN, 0, 0, 0]] * c.rows
    assert (c.d.download() == c.x).all()
    eng.check()


def _patterns(c, r, j):
    """name -> bits to flip in word j of row r (odd, below q / 2)"""
    x = int(c.x[r, j])
    assert x & 1 and x < c.q_of[r] // 2 + 1
    return {"one bit": [3], "three bits": [1, 30, 47], "x + p": [0, 61], "pushed past q": [62]}


@pytest.mark.parametrize("logn", LOGNS)
def test_one_corrupted_word_per_row_is_restored_exactly(eng, rows_of, logn):
    c = rows_of(logn)
    N, last = c.N, c.rows - 1
    # first, middle and last row (each at another spot of its row), and two rows at once
    targets = [{0: c.spots[0]}, {c.rows // 2: c.spots[1]}, {last: c.spots[2]}, {0: c.spots[2], last: c.spots[1]}]
    for name in ("one bit", "three bits", "x + p", "pushed past q"):
        for tg in targets:
            want_rep = {}
            for r, j in tg.items():
                bits = _patterns(c, r, j)[name]
                for b in bits:
                    flip(eng, c.d, r * N + j, b)
                bad = int(c.x[r, j])
                for b in bits:
                    bad ^= 1 << b
                want_rep[r] = [REPAIRED, j, bad, int(c.x[r, j])]
                if name == "x + p":
                    assert bad == int(c.x[r, j]) + P
                if name == "pushed past q":
                    assert bad >= c.q_of[r]
            # the verifying call alone still raises exactly these rows, and writes nothing
            seen = c.t.seal_verify(c.d, c.seal, **c.kw).tolist()
            assert [r for r in range(c.rows) if seen[r]] == sorted(tg), (name, tg, seen)
            if name == "x + p":
                assert all(seen[r] == RANGE for r in tg), seen      # no sum moves: the window alone
            flags, report = c.repair()
            assert report.tolist() == c.only(want_rep, None, 4), (name, tg, report.tolist())
            assert flags.tolist() == [0] * c.rows, (name, tg)
            assert (c.d.download() == c.x).all(), (name, tg)
    assert not c.t.seal_verify(c.d, c.seal, **c.kw).any()
    eng.check()


def _traps(c, r):
    """name -> [(word, bit)] flips in row r that change exactly two words and stay in the window"""
    a, b = int(c.x[r, 5]), int(c.x[r, 20])
    assert a ^ b == 0b101
    return {
        "midpoint": [(2, 7), (10, 7)],                              # the same bit set in words 2 and 10: two sums name word 6
        "d2 = -2 d1": [(4, 7), (9, 8)],                             # +2^7 in word 4, -2^8 in word 9: two sums name word 14
        "swapped": [(5, 0), (5, 2), (20, 0), (20, 2)],              # words 5 and 20 exchanged: S0 does not move
    }


@pytest.mark.parametrize("logn", LOGNS)
def test_two_corrupted_words_in_a_row_are_never_written_to(eng, rows_of, logn):
    c = rows_of(logn)
    N = c.N
    for r in (0, c.rows - 1):
        for name, flips in _traps(c, r).items():
            y = c.x.copy()
            for j, b in flips:
                flip(eng, c.d, r * N + j, b)
                y[r, j] ^= np.uint64(1 << b)
            assert int((y[r] != c.x[r]).sum()) == 2 and (y[r] < np.uint64(c.q_of[r])).all()
            if name == "midpoint":
                assert int(y[r, 2]) - int(c.x[r, 2]) == int(y[r, 10]) - int(c.x[r, 10]) == 1 << 7
            if name == "d2 = -2 d1":
                assert int(y[r, 4]) - int(c.x[r, 4]) == 1 << 7 and int(y[r, 9]) - int(c.x[r, 9]) == -(1 << 8)
            if name == "swapped":
                assert y[r, 5] == c.x[r, 20] and y[r, 20] == c.x[r, 5]
            try:
                flags, report = c.repair()
                assert report.tolist() == c.only([r], [UNCORRECTABLE, 0, 0, 0], 4), (name, r, report.tolist())
                assert flags.tolist() == c.only([r], SUM), (name, r)
                assert c.d.download().tobytes() == y.tobytes(), (name, r)      # byte-identical to the corrupted state
            finally:
                for j, b in flips:
                    flip(eng, c.d, r * N + j, b)
    assert (c.d.download() == c.x).all() and not c.repair()[0].any()
    eng.check()


@pytest.mark.parametrize("logn", [5, 14])
def test_a_corrupted_seal_or_locator_word_never_causes_a_write(eng, rows_of, logn):
    c = rows_of(logn)
    N, r = c.N, c.rows // 2
    x_bytes = c.x.tobytes()
    # one stored sum of the seal: the row is intact, one syndrome is non-zero
    for word in (2 * r, 2 * r + 1):
        flip(eng, c.seal, word, 21)
        try:
            flags, report = c.repair()
            assert report.tolist() == c.only([r], [SUSPECT, 0, 0, 0], 4) and flags.tolist() == c.only([r], SUM), word
            assert c.d.download().tobytes() == x_bytes
        finally:
            flip(eng, c.seal, word, 21)
    # the locator word beside an intact row and seal: the verifying sweep raises nothing, so the row is not examined
    flip(eng, c.loc, r, 21)
    try:
        flags, report = c.repair()
        assert not flags.any() and report.tolist() == [[CLEAN, 0, 0, 0]] * c.rows and c.d.download().tobytes() == x_bytes
        # ... beside a corrupted seal word: two sums moved
        flip(eng, c.seal, 2 * r, 40)
        try:
            flags, report = c.repair()
            assert report.tolist() == c.only([r], [UNCORRECTABLE, 0, 0, 0], 4) and flags.tolist() == c.only([r], SUM)
            assert c.d.download().tobytes() == x_bytes
        finally:
            flip(eng, c.seal, 2 * r, 40)
        # ... beside one corrupted word of the row, which a good locator would have repaired: inconsistent syndromes
        j = c.spots[1]
        flip(eng, c.d, r * N + j, 3)
        try:
            y = c.x.copy()
            y[r, j] ^= np.uint64(8)
            flags, report = c.repair()
            assert report.tolist() == c.only([r], [UNCORRECTABLE, 0, 0, 0], 4) and flags.tolist() == c.only([r], SUM)
            assert c.d.download().tobytes() == y.tobytes()
        finally:
            flip(eng, c.d, r * N + j, 3)
    finally:
        flip(eng, c.loc, r, 21)
    # a corrupted seal word beside one corrupted word of the row
    j = c.spots[2]
    flip(eng, c.seal, 2 * r + 1, 5)
    flip(eng, c.d, r * N + j, 3)
    try:
        y = c.x.copy()
        y[r, j] ^= np.uint64(8)
        flags, report = c.repair()
        assert report.tolist() == c.only([r], [UNCORRECTABLE, 0, 0, 0], 4) and flags.tolist() == c.only([r], SUM)
        assert c.d.download().tobytes() == y.tobytes()
    finally:
        flip(eng, c.seal, 2 * r + 1, 5)
        flip(eng, c.d, r * N + j, 3)
    flags, report = c.repair()
    assert not flags.any() and c.d.download().tobytes() == x_bytes
    eng.check()


@pytest.mark.parametrize("logn", [5, 14, 17])
def test_the_register_hook_is_a_transient(eng, rows_of, logn):
    from fhe_reliability_gpu_amd._lib import check, lib
    c = rows_of(logn)
    for r, j, bit in ((0, 0, 3), (c.rows - 1, c.N - 1, 62), (c.rows // 2, c.mid, 17)):
        check(lib.fhe_ctx_inject_fault_seal(eng._h, r, j, bit))
        flags, report = c.repair()
        assert report.tolist() == c.only([r], [TRANSIENT, 0, 0, 0], 4), (r, j, bit, report.tolist())
        assert not flags.any()
        assert (c.d.download() == c.x).all()
        # one shot
        flags, report = c.repair()
        assert not flags.any() and report.tolist() == [[CLEAN, 0, 0, 0]] * c.rows
    # the hook beside a word that is corrupted in memory, in another row: one transient, one repair
    r, j = c.rows - 1, c.spots[1]
    flip(eng, c.d, r * c.N + j, 9)
    check(lib.fhe_ctx_inject_fault_seal(eng._h, 0, 5, 3))
    flags, report = c.repair()
    assert report.tolist() == c.only({0: [TRANSIENT, 0, 0, 0], r: [REPAIRED, j, int(c.x[r, j]) ^ 512, int(c.x[r, j])]}, None, 4)
    assert not flags.any() and (c.d.download() == c.x).all()
    eng.check()


def test_a_repair_inside_a_stream_capture(F, eng, rows_of):
    import torch
    from fhe_reliability_gpu_amd._lib import check, lib
    c = rows_of(14)
    N, r, j = c.N, c.rows - 1, c.spots[1] + 1
    flags = torch.full((c.rows,), 0x5A5A5A5A, device="cuda", dtype=torch.int32)
    report = torch.full((c.rows, 4), 0x5A5A5A5A, device="cuda", dtype=torch.int64)
    ptr = lambda x: C.c_void_p(x.data_ptr())

    def call(s):
        check(lib.fhe_seal_repair(eng._h, c.d.ptr, c.seal.ptr, c.loc.ptr, c.t._h, c.n_poly, c.limbs, c.start, ptr(flags), ptr(report),
                                  C.c_void_p(s.cuda_stream)))

    s = torch.cuda.Stream()
    call(s)      # the warm-up: the context's scratch exists from here on
    torch.cuda.synchronize()
    assert not flags.any() and not report.any()
    graph, cap = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=cap):
        call(cap)
    flip(eng, c.d, r * N + j, 44)
    eng.sync()
    assert c.t.seal_verify(c.d, c.seal, **c.kw).tolist() == c.only([r], SUM)
    graph.replay()
    torch.cuda.synchronize()
    bad = int(c.x[r, j]) ^ (1 << 44)
    assert report.tolist() == c.only([r], [REPAIRED, j, bad, int(c.x[r, j])], 4) and not flags.any()
    assert (c.d.download() == c.x).all()
    graph.replay()      # and again, on the repaired rows
    torch.cuda.synchronize()
    assert not report.any() and not flags.any()
    eng.check()


def test_repair_argument_rules(F, eng, rows_of):
    from fhe_reliability_gpu_amd._lib import check, lib
    c = rows_of(13)
    h, t = eng._h, c.t._h
    fl = eng.upload(np.full(c.rows, GARBAGE, dtype=np.uint64))
    rp = eng.upload(np.full(4 * c.rows, GARBAGE, dtype=np.uint64))
    lo = eng.upload(np.full(c.rows, GARBAGE, dtype=np.uint64))
    args = lambda **k: [k.get("d", c.d.ptr), k.get("seal", c.seal.ptr), k.get("loc", c.loc.ptr), t, k.get("n_poly", c.n_poly), k.get("limbs", c.limbs),
                        k.get("start", c.start), k.get("flags", fl.ptr), k.get("report", rp.ptr), None]
    # nothing to do: FHE_OK, nothing touched
    for n_poly, limbs in ((0, 2), (1, 0)):
        check(lib.fhe_seal_repair(h, *args(n_poly=n_poly, limbs=limbs)))
        check(lib.fhe_seal_locator(h, lo.ptr, c.d.ptr, t, n_poly, limbs, 0, None))
    # null locator or report, and the verifying call's rules: null words / seal / flags, a window outside the table set, misalignment
    for bad in (dict(loc=None), dict(report=None), dict(d=None), dict(seal=None), dict(flags=None), dict(start=len(c.qs) - 1),
                dict(limbs=len(c.qs) + 1, start=0), dict(d=C.c_void_p(c.d.ptr.value + 8)), dict(report=C.c_void_p(rp.ptr.value + 8))):
        assert lib.fhe_seal_repair(h, *args(**bad)) == INVALID, bad
    assert lib.fhe_seal_locator(h, None, c.d.ptr, t, 1, 1, 0, None) == INVALID and lib.fhe_seal_locator(h, lo.ptr, None, t, 1, 1, 0, None) == INVALID
    assert lib.fhe_seal_locator(h, lo.ptr, c.d.ptr, t, 1, 2, len(c.qs) - 1, None) == INVALID
    assert lib.fhe_seal_locator(h, lo.ptr, C.c_void_p(c.d.ptr.value + 8), t, 1, 1, 0, None) == INVALID
    # a hook outside the call: refused, nothing launched, used up
    for row, coeff in ((c.rows, 0), (0, c.N)):
        check(lib.fhe_ctx_inject_fault_seal(h, row, coeff, 0))
        assert lib.fhe_seal_repair(h, *args()) == INVALID
    assert (fl.download() == GARBAGE).all() and (rp.download() == GARBAGE).all() and (lo.download() == GARBAGE).all()
    check(lib.fhe_seal_repair(h, *args()))
    assert not fl.download().view(np.uint32)[:c.rows].any() and not rp.download().any()
    # the locator call leaves an armed hook to the next verifying call
    check(lib.fhe_ctx_inject_fault_seal(h, 1, 5, 0))
    assert c.t.seal_locator(c.d, **c.kw).download().tolist() == [w[2] for w in c.want]
    assert c.repair()[1].tolist() == c.only([1], [TRANSIENT, 0, 0, 0], 4)
    assert (c.d.download() == c.x).all()
    eng.check()


# ---------------------------------------------------------------------------------------------------------------- composites
class Case(SealedCase):
    """the 2^13 plan, seeded operands on the host and on the device, their seals and locators"""

    def __init__(self, F, eng):
        super().__init__(F, eng, (13, 3, 1, 3, limb_bits("mixed", 3, 1)), seed=14, margin=0)
        self.locs = [self.t.seal_locator(v, limbs=self.L) for v in self.d]
        self.key_loc = self.ks.seal_key_locator(self.dk)
        for v, s, l in zip(self.ops + [self.key], self.seals + [self.key_seal], self.locs + [self.key_loc]):
            want = py_seals_and_locator(v)
            assert s.download().tolist() == [w[:2] for w in want] and l.download().tolist() == [w[2] for w in want]


@pytest.fixture(scope="module")
def case(F, eng):
    return Case(F, eng)


def _outcomes(reports):
    """[(name, flat row, record)] of every row whose outcome is not CLEAN"""
    out = []
    for name, rep in reports.items():
        flat = np.asarray(rep).reshape(-1, 4)
        out += [(name, int(r), flat[r].tolist()) for r in np.flatnonzero(flat[:, 0])]
    return out


def _words(*arrays):
    return [a.download().tolist() for a in arrays]


@pytest.mark.parametrize("tp", [0, 65537])
def test_repairing_composites_correct_a_flipped_word_and_give_the_clean_results(F, eng, case, tp):
    c = case
    ks, ab, L, N, M = c.ks, c.ab, c.L, c.N, c.M
    gal = 5
    with plain_modulus(ks, tp):
        lay, rlay = ks.hmult_sealed_repair_layout(True), ks.hmult_sealed_layout(True)
        assert all(lay[k] == rlay[k] for k in ("a0", "a1", "b0", "b1", "key", "checked")) and lay["flags_total"] == rlay["total"]
        assert lay["report"] % 4 == 0 and lay["total"] == lay["report"] + 8 * lay["checked"]
        pairs = dict(seals=c.seals, locators=c.locs, key_seal=c.key_seal, key_locator=c.key_loc)
        hm_clean = ks.hmult_sealed(*c.d, c.dk, ab, seals=c.seals, key_seal=c.key_seal)
        rot_clean = ks.rotate_sealed(c.d[0], c.d[1], gal, c.dk, ab, seals=c.seals[:2], key_seal=c.key_seal)
        assert raised(hm_clean[3]) == [] and raised(rot_clean[3]) == []
        hm_want, rot_want = _words(hm_clean[0], hm_clean[1], *hm_clean[2]), _words(rot_clean[0], rot_clean[1], *rot_clean[2])

        def hmult_repair():
            return ks.hmult_sealed_repair(*c.d, c.dk, ab, **pairs)

        def rotate_repair():
            return ks.rotate_sealed_repair(c.d[0], c.d[1], gal, c.dk, ab, seals=c.seals[:2], locators=c.locs[:2], key_seal=c.key_seal, key_locator=c.key_loc)

        # a clean repairing call: the sealed call's words and seals, no flag, every report CLEAN, and the outputs' locators
        for got, want in ((hmult_repair(), hm_want), (rotate_repair(), rot_want)):
            o0, o1, so, lo, fl, rep = got
            assert _words(o0, o1, *so) == want and raised(fl) == [] and _outcomes(rep) == []
            for o, l in zip((o0, o1), lo):
                limbs = o.size // N
                assert l.download().tolist() == [w[2] for w in py_seals_and_locator(o.download().reshape(limbs, N))]
                assert l.download().tolist() == c.t.seal_locator(o, limbs=limbs).download().tolist()
        key_row = (1 * 2 + 1) * M + (M - 1)                      # digit 1, half 1, the special limb
        targets = [("a0", c.d[0], L - 1, c.ops[0][L - 1], c.qs[L - 1]), ("key", c.dk, key_row, c.key[1, 1, M - 1], c.qs[M - 1])]
        for what, dev, row, words, q in targets:
            j = safe_coeff(words, q, N // 2 + 7, room=64)      # bits 3 and 4 flip
            rwhat = "c0" if what == "a0" else "key"
            record = [REPAIRED, j, int(words[j]) ^ 8, int(words[j])]
            for sealed, repairing, name, want in ((lambda: ks.hmult_sealed(*c.d, c.dk, ab, seals=c.seals, key_seal=c.key_seal), hmult_repair, what, hm_want),
                                                  (lambda: ks.rotate_sealed(c.d[0], c.d[1], gal, c.dk, ab, seals=c.seals[:2], key_seal=c.key_seal),
                                                   rotate_repair, rwhat, rot_want)):
                flip(eng, dev, row * N + j, 3)
                # the verifying composite, unchanged: it raises the row and computes on what it was given
                fl = sealed()[3]
                assert raised({k: v for k, v in fl.items() if k != "checked"}) == [(name, row)]
                assert not c.unchanged()
                # the repairing composite: the clean call's words and output seals, no flag raised anywhere, the word named
                o0, o1, so, lo, fl, rep = repairing()
                assert raised(fl) == [], (what, name, raised(fl))
                assert _outcomes(rep) == [(name, row, record)], (what, name, _outcomes(rep))
                assert _words(o0, o1, *so) == want, (what, name)
                assert c.unchanged()
            # two words of that row: the row is raised, reported UNCORRECTABLE and left as it was found; the call goes on
            flip(eng, dev, row * N + j, 3)
            flip(eng, dev, row * N + j + 1, 4)
            try:
                before = dev.download().tobytes()
                for repairing, name in ((hmult_repair, what), (rotate_repair, rwhat)):
                    fl, rep = repairing()[4:]
                    assert raised({k: v for k, v in fl.items() if k != "checked"}) == [(name, row)]
                    assert _outcomes(rep) == [(name, row, [UNCORRECTABLE, 0, 0, 0])]
                    assert dev.download().tobytes() == before
            finally:
                flip(eng, dev, row * N + j, 3)
                flip(eng, dev, row * N + j + 1, 4)
            assert c.unchanged()
    eng.check()


def test_repairing_composites_take_seal_and_locator_together(F, eng, case):
    from fhe_reliability_gpu_amd._lib import lib, vp
    c = case
    ks, ab, N, L = c.ks, c.ab, c.N, c.L
    o0, o1 = eng.alloc(L * N), eng.alloc(L * N)
    words = ks.hmult_sealed_repair_layout(True)["total"] // 2
    sin, lin = (vp * 4)(*[s.ptr for s in c.seals]), (vp * 4)(*[s.ptr for s in c.locs])
    d = c.d

    def both(seal_in, loc_in, key_seal, key_loc, flags):
        return [lib.fhe_hmult_sealed_repair(eng._h, ks._h, o0.ptr, o1.ptr, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, c.dk.ptr, 1, ab._h, seal_in, loc_in, key_seal,
                                            key_loc, None, None, flags, None),
                lib.fhe_rotate_sealed_repair(eng._h, ks._h, o0.ptr, o1.ptr, d[0].ptr, d[1].ptr, 5, c.dk.ptr, ab._h, seal_in, loc_in, key_seal, key_loc, None,
                                             None, flags, None)]

    fl = eng.upload(np.full(words, GARBAGE, dtype=np.uint64))
    half = (vp * 4)(c.locs[0].ptr, None, c.locs[2].ptr, c.locs[3].ptr)
    for a in ((sin, None, None, None), (sin, half, None, None), (None, lin, None, None), (sin, lin, c.key_seal.ptr, None),
              (sin, lin, None, c.key_loc.ptr)):
        assert both(*a, fl.ptr) == [INVALID] * 2
        assert (fl.download() == GARBAGE).all()      # nothing launched
    assert both(sin, lin, c.key_seal.ptr, c.key_loc.ptr, C.c_void_p(fl.ptr.value + 8)) == [INVALID] * 2      # the report block is 16-byte aligned
    assert both(sin, lin, c.key_seal.ptr, c.key_loc.ptr, None) == [INVALID] * 2
    assert (fl.download() == GARBAGE).all()
    # no pair at all, or some: fine
    assert both(None, None, None, None, fl.ptr) == [0, 0]
    none1 = (vp * 4)(c.seals[0].ptr, None, c.seals[2].ptr, c.seals[3].ptr)
    assert both(none1, half, c.key_seal.ptr, c.key_loc.ptr, fl.ptr) == [0, 0]
    assert c.unchanged()
    eng.check()
