"""What the GPU tests of the sealed transforms share (test_gpu_ntt_fwd_sealed.py at the sizes where a code path first exists,
test_gpu_sealed_sizes.py at every size): the seeded case of one shape, the runners of the clean call, of corruptions at rest and of
the fault between the launches, and -- for the every-size file -- the seal held against Python integers and a hook sweep over words
chosen without knowledge of the tile geometry.  Every comparison is ==."""
import numpy as np

from helpers.sealed_case import flip, py_seals

INVALID, UNSUPPORTED = 1, 3
SUM, RANGE = 1, 2
POISON = (1 << 64) - 1
GARBAGE = 0x5A5A5A5A5A5A5A5A


class Case:
    """a table set, its detector, seeded rows [n_poly][limbs][N] in both domains on the host and on the device, their seals.
    shape = (limb bits of the table set, n_poly, start_idx)"""

    def __init__(self, F, eng, logn, shape):
        bits, self.n_poly, self.start = shape
        self.logn, self.N = logn, 1 << logn
        self.qs = F.create_moduli(self.N, bits)
        self.limbs = len(bits) - self.start
        self.rows = self.n_poly * self.limbs
        self.kw = dict(limbs=self.limbs, start=self.start, n_poly=self.n_poly)
        self.t = eng.tables(logn, self.qs)
        self.ab = F.Abft(eng, self.t)
        rng = np.random.default_rng(1000 + logn)
        self.q_of = [self.qs[self.start + r % self.limbs] for r in range(self.rows)]
        self.x = np.stack([rng.integers(16, q - 16, self.N, dtype=np.uint64) for q in self.q_of])
        self.d = eng.upload(self.x)
        self.seal = self.t.seal(self.d, **self.kw)
        # the references, computed once: the unchecked forward transform of x, its seal, and both as the inverse's input
        self.dX = self.unchecked(eng, self.d, False)
        self.X = self.dX.download().reshape(self.rows, self.N)
        self.seal_X = self.t.seal(self.dX, **self.kw)

    def unchecked(self, eng, src, inv):
        w = eng.alloc(self.rows * self.N)
        w.copy_from(src)
        (self.t.inverse if inv else self.t.forward)(w, **self.kw)
        return w

    def side(self, inv):
        """(call, source, its seal, host words of the source, host words of the result)"""
        if inv:
            return self.t.intt_sealed_out, self.dX, self.seal_X, self.X, self.x
        return self.t.ntt_sealed, self.d, self.seal, self.x, self.X

    def seals_of(self, dst):
        return self.t.seal(dst, **self.kw).download().reshape(self.rows, 2)

    def words(self):
        """(row, word): word 0, both sides of the middle of a row (a tile edge of the row passes from 2^13 on), the last word"""
        return [(0, 0), (self.rows - 1, self.N // 2 - 1), (self.rows // 2, self.N // 2), (self.rows - 1, self.N - 1)]


def rows_of(dst, c):
    return dst.download().reshape(c.rows, c.N)


def check_raised(c, eng, dst, seal_dst, fl, rows, block):
    """exactly `rows` raised in `block` and nothing in the other one; exactly their seals poisoned, every other row's seal fhe_seal's;
    a sweep of dst against seal_dst raises them and no other row"""
    rows = sorted(rows)
    assert np.flatnonzero(fl[block]).tolist() == rows and not fl[1 - block].any(), fl
    s = seal_dst.download().reshape(c.rows, 2)
    want = c.seals_of(dst)
    for r in range(c.rows):
        assert s[r].tolist() == ([POISON, POISON] if r in rows else want[r].tolist()), r
    assert np.flatnonzero(c.t.seal_verify(dst, seal_dst, **c.kw)).tolist() == rows


def flips_scenarios(c, host):
    """[(name, [(row, word, bit)], rows that must carry SEAL_RANGE)]: single bits 0, 40 and 63; the reference's pattern, 3 symbols x 4
    bits in one row and spread over two rows; one word moved by +2^b - 2^(b + 32)"""
    r0, r1 = c.rows - 1, c.rows // 2 if c.rows // 2 != c.rows - 1 else 0
    N = c.N
    out = [("bit0", [(r0, 0, 0)], []), ("bit40", [(r1, N // 2, 40)], None), ("bit63", [(r0, N - 1, 63)], [r0])]
    sym = [(5, [1, 9, 17, 33]), (N // 2 + 3, [0, 13, 22, 47]), (N - 2, [2, 3, 30, 44])]
    out.append(("3x4 one row", [(r1, j, b) for j, bs in sym for b in bs], None))
    out.append(("3x4 two rows", [((r0, r1, r0)[i], j, b) for i, (j, bs) in enumerate(sym) for b in bs], None))
    b = 7
    j = next(j for j in range(N // 3, N) if not (int(host[r1][j]) >> b) & 1 and (int(host[r1][j]) >> (b + 32)) & 1)
    out.append(("fold-blind", [(r1, j, b), (r1, j, b + 32)], []))
    return out


def run_flips(c, eng, inv):
    call, src0, seal, host, _ = c.side(inv)
    src = eng.alloc(c.rows * c.N)
    src.copy_from(src0)
    for name, flips, ranged in flips_scenarios(c, host):
        for r, j, b in flips:
            flip(eng, src, r * c.N + j, b)
        try:
            dst, seal_dst, fl = call(src, seal, c.ab, **c.kw)
            want = c.unchecked(eng, src, inv)
        finally:
            for r, j, b in flips:
                flip(eng, src, r * c.N + j, b)
        rows = {r for r, _, _ in flips}
        check_raised(c, eng, dst, seal_dst, fl, rows, 0)
        assert all(int(fl[0][r]) & SUM for r in rows), (name, fl)
        if ranged is not None:
            assert [r for r in range(c.rows) if int(fl[0][r]) & RANGE] == ranged, (name, fl)
        assert (rows_of(dst, c) == rows_of(want, c)).all(), name      # the transform of the source as it is
    assert (src.download().reshape(-1) == src0.download().reshape(-1)).all()


def run_clean(c, eng, inv):
    call, src, seal, host, ref = c.side(inv)
    dst, seal_dst, fl = call(src, seal, c.ab, **c.kw)
    assert fl.shape == (2, c.rows) and not fl.any()
    assert (rows_of(dst, c) == ref).all()
    assert (src.download().reshape(c.rows, c.N) == host).all()              # out of place: the source is only read
    assert (seal_dst.download().reshape(c.rows, 2) == c.seals_of(dst)).all()
    w = eng.alloc(c.rows * c.N)
    w.copy_from(src)
    same_buf, seal_w, fl = call(w, seal, c.ab, dst=w, **c.kw)
    assert same_buf is w and not fl.any() and (rows_of(w, c) == ref).all()
    assert (seal_w.download() == seal_dst.download()).all()
    # no output seal asked for: none comes back, words and flags are the same
    dst, none, fl = call(src, seal, c.ab, seal_out=False, **c.kw)
    assert none is None and not fl.any() and (rows_of(dst, c) == ref).all()
    # a stored seal that is wrong raises its row; without one nothing is compared
    bad = seal.download().copy().reshape(c.rows, 2)
    bad[c.rows - 1] = GARBAGE
    dst, seal_dst, fl = call(src, eng.upload(bad), c.ab, **c.kw)
    check_raised(c, eng, dst, seal_dst, fl, [c.rows - 1], 0)
    dst, seal_dst, fl = call(src, None, c.ab, **c.kw)
    assert not fl.any() and (seal_dst.download().reshape(c.rows, 2) == c.seals_of(dst)).all()
    eng.check()


def run_between(c, eng, inv):
    from fhe_reliability_gpu_amd._lib import check, lib
    call, src, seal, _, ref = c.side(inv)
    row, j = c.rows - 1, c.N // 2 + 5
    check(lib.fhe_ctx_inject_fault(eng._h, row * c.N + j, 30))
    dst, seal_dst, fl = call(src, seal, c.ab, **c.kw)
    check_raised(c, eng, dst, seal_dst, fl, [row], 1)
    assert not (rows_of(dst, c) == ref).all()
    dst, seal_dst, fl = call(src, seal, c.ab, **c.kw)      # one shot
    assert not fl.any() and (rows_of(dst, c) == ref).all()
    eng.check()


def run_inverse_without_output_seal(c, eng):
    """intt_sealed, the inverse that writes no output seal: clean words and flags, and under the hook the words and flags of
    intt_sealed_out under the same hook -- the transform of the flipped word"""
    dst, fl = c.t.intt_sealed(c.dX, c.seal_X, c.ab, **c.kw)
    assert not fl.any() and (rows_of(dst, c) == c.x).all()
    row, j = c.rows - 1, c.N // 2
    eng.inject_fault_ntt_sealed(row, j, 3)
    hooked, fl = c.t.intt_sealed(c.dX, c.seal_X, c.ab, **c.kw)
    assert np.flatnonzero(fl[0]).tolist() == [row] and int(fl[0][row]) == SUM and not fl[1].any()
    # the same fault through the call with an output seal: the same words and flags
    eng.inject_fault_ntt_sealed(row, j, 3)
    out, seal_out, fl2 = c.t.intt_sealed_out(c.dX, c.seal_X, c.ab, **c.kw)
    assert (fl2 == fl).all() and (rows_of(out, c) == rows_of(hooked, c)).all()
    # and what the fault computes is the transform of the flipped word
    y = eng.alloc(c.rows * c.N)
    y.copy_from(c.dX)
    flip(eng, y, row * c.N + j, 3)
    assert (rows_of(hooked, c) == rows_of(c.unchecked(eng, y, True), c)).all()
    eng.check()


# ---- the every-size additions ----

def pow2_words(logn):
    """words 2^k - 1 and 2^k for k = 0 .. logn - 1, and word N - 1, each once: every tile edge of every plan lies at a multiple of a
    power of two, so this set holds a word on both sides of the first edge of any tile size"""
    ws = [w for k in range(logn) for w in ((1 << k) - 1, 1 << k)] + [(1 << logn) - 1]
    return list(dict.fromkeys(ws))


def sampled_rows(c):
    """the rows held against Python integers: every row below 2^17, row 0 and the last row from there on (a row of 2^20 words takes
    about a second on the host)"""
    return list(range(c.rows)) if c.logn < 17 else [0, c.rows - 1]


def run_clean_python_seal(c, eng, inv):
    """the output seal of a clean call is the Python-integer seal of the unchecked transform's words, out of place and in place"""
    call, src, seal, _, ref = c.side(inv)
    rows = sampled_rows(c)
    want = py_seals(ref[rows])
    dst, seal_dst, fl = call(src, seal, c.ab, **c.kw)
    assert not fl.any() and (rows_of(dst, c) == ref).all()
    assert seal_dst.download().reshape(c.rows, 2)[rows].tolist() == want
    w = eng.alloc(c.rows * c.N)
    w.copy_from(src)
    _, seal_w, fl = call(w, seal, c.ab, dst=w, **c.kw)
    assert not fl.any() and seal_w.download().reshape(c.rows, 2)[rows].tolist() == want
    eng.check()


def run_hook_sweep(c, eng, inv):
    """the hook on every word of pow2_words, alternating between row 0 and the last row: exactly that row raised with SEAL_SUM and
    poisoned, memory unchanged, the output words those of the unchecked transform of a copy with that one bit flipped -- which proves
    the hook hit word j and not another word of the same tile -- and the next call clean"""
    call, src, seal, host, ref = c.side(inv)
    w = eng.alloc(c.rows * c.N)
    for i, j in enumerate(pow2_words(c.logn)):
        row = (0, c.rows - 1)[i & 1]
        eng.inject_fault_ntt_sealed(row, j, 3)
        dst, seal_dst, fl = call(src, seal, c.ab, **c.kw)
        check_raised(c, eng, dst, seal_dst, fl, [row], 0)
        assert int(fl[0][row]) == SUM, (row, j, fl)
        assert (rows_of(src, c) == host).all(), (row, j)                     # memory is clean
        w.copy_from(src)
        flip(eng, w, row * c.N + j, 3)
        (c.t.inverse if inv else c.t.forward)(w, **c.kw)
        got = rows_of(dst, c)
        assert (got == rows_of(w, c)).all(), (row, j)
        assert not (got[row] == ref[row]).all(), (row, j)
        dst, seal_dst, fl = call(src, seal, c.ab, **c.kw)                    # one shot
        assert not fl.any() and (rows_of(dst, c) == ref).all(), (row, j)
    eng.check()
