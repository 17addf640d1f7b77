"""The natural-order transform on the inputs of tests/helpers/gs_worst_case.py -- pulses for every stage of its own network, the
constant and alternating patterns laid on its pair structure, spikes and words next to q, for the largest 50-bit prime that is
1 mod N and a 30-bit one, forward and inverse -- through fhe_ntt_cyclic, the four-step calls (plain, batch, checked, per phase) and
the sub-batched pipeline; the small and unusual moduli of tests/helpers/cyclic_cases.py through F.ntt / F.intt / F.four_step_ntt; and
fhe_ntt_forward_inplace / fhe_ntt_inverse_inplace called directly.  Every comparison is == against the oracle.

Sizes: 2^5, 2^9, 2^12 (one, two, three register steps), 2^13 / 2^14 (the first two-launch sizes), 2^16, 2^17 / 2^18 (three-step rows)."""
import numpy as np
import pytest

from test_gpu_subbatch import small_chunks  # noqa: F401  (1 MiB sub-batches, the defaults restored afterwards)
from helpers import cyclic_cases as K
from helpers import gs_worst_case as G

pytestmark = pytest.mark.gpu

SIZES = [5, 9, 12, 13, 14, 16, 17, 18]


@pytest.fixture(scope="module")
def F():
    import fhe_reliability_gpu_amd as f
    return f


@pytest.fixture(scope="module")
def eng(F):
    return F.default_engine()


@pytest.fixture(scope="module")
def O():
    from oracle import cport
    return cport


_CASES = {}


def designed(logn, bits):
    """The designed batch of one size and prime: names, forward inputs with their oracle images, inverse inputs with theirs.
    Computed once, shared, never modified.  At 2^18 the pulses of stages 0, 1, logn/2, logn-1 plus the soak set."""
    if (logn, bits) not in _CASES:
        pulses = (0, 1, logn // 2, logn - 1) if logn >= 18 else None
        c = {}
        for inverse in (False, True):
            L = G.GsLimb(logn, bits, inverse)
            fam = G.families(L, pulses=pulses)
            data = np.stack([v for _, v, *_ in fam])
            want = np.stack([L.oracle(v) for v in data])
            data.setflags(write=False), want.setflags(write=False)
            c["inv" if inverse else "fwd"] = dict(L=L, names=[n for n, *_ in fam], data=data, want=want)
        _CASES[logn, bits] = c
    return _CASES[logn, bits]


def _bad(c, got):
    return [n for n, g, w in zip(c["names"], got.reshape(c["want"].shape), c["want"]) if not (g == w).all()]


def _cyclic(eng, x, logn, q, g, inverse):
    from fhe_reliability_gpu_amd._lib import check, lib
    d, s = eng.upload(x), eng.alloc(x.size)
    check(lib.fhe_ntt_cyclic(eng._h, d.ptr, s.ptr, logn, x.shape[0], q, g, 0, inverse, None))
    out = d.download().reshape(x.shape)
    d.free(), s.free()
    return out


@pytest.mark.parametrize("bits", [50, 30])
@pytest.mark.parametrize("logn", SIZES)
def test_cyclic_forward_inverse_and_round_trip(eng, logn, bits):
    c = designed(logn, bits)
    f, i = c["fwd"], c["inv"]
    q, g = f["L"].q, f["L"].g
    eng.trace(True)
    try:
        got = _cyclic(eng, f["data"], logn, q, g, 0)
        assert _bad(f, got) == []
        assert (_cyclic(eng, got, logn, q, g, 1) == f["data"]).all()              # the round trip
        got = _cyclic(eng, i["data"], logn, q, g, 1)
        assert _bad(i, got) == []
        assert (_cyclic(eng, got, logn, q, g, 0) == i["data"]).all()
    finally:
        eng.trace(False)
    # all four calls, the inverse root's included, went through the natural-order launches -- the code these vectors are built for --
    # and none through the forward-network route, which would give the same words
    text = eng.trace_text()
    assert text.count("NTT_CYCLIC_NATURAL_ORDER") == 4 and "NTT_CYCLIC_FORWARD_NETWORK" not in text, text
    eng.check()


@pytest.mark.parametrize("bits", [50, 30])
@pytest.mark.parametrize("n1,n2", [(16, 32), (64, 128), (256, 256), (512, 256)])
def test_fourstep_calls_on_designed_vectors(F, eng, O, n1, n2, bits):
    """ntt (one vector), the batch call, ntt_checked and ntt_checked_phases: the same words, every flag present and zero"""
    from fhe_reliability_gpu_amd._lib import FheError
    logn = (n1 * n2).bit_length() - 1
    f = designed(logn, bits)["fwd"]
    q, g, x, P = f["L"].q, f["L"].g, f["data"], len(f["names"])
    assert (f["want"][0] == O.four_step_ntt(x[0], n1, n2, q, g)).all()
    assert F.four_step_ntt(x[0], n1 * n2, q, g, n1=n1) == f["want"][0].tolist()
    fs = F.FourStep(eng, n1, n2, q, g)
    src, dst = eng.upload(x), eng.alloc(x.size)
    fs.ntt(src, dst, P)
    assert _bad(f, dst.download()) == []
    dst2 = eng.alloc(x.size)
    flags = fs.ntt_checked(src, dst2, P)
    assert _bad(f, dst2.download()) == []
    assert flags.shape == (P,) and not flags.any()
    dst3 = eng.alloc(x.size)
    if logn >= 13:
        flags = fs.ntt_checked_phases(src, dst3, P)
        assert _bad(f, dst3.download()) == []
        assert flags.shape == (P, 3) and not flags.any()
    else:
        with pytest.raises(FheError):                   # single-launch sizes have one phase: a status, not a transform
            fs.ntt_checked_phases(src, dst3, P)
    fs.close()
    eng.check()


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("logn", [13, 16])
def test_designed_batch_cut_into_sub_batches(F, eng, small_chunks, logn, split):
    """the designed batch past the sub-batch size: pieces on one stream and on alternating streams, plain and checked"""
    eng.set_option("ntt_split", split)
    for bits in (50, 30):
        c = designed(logn, bits)
        f, i = c["fwd"], c["inv"]
        q, g, P = f["L"].q, f["L"].g, len(f["names"])
        assert f["data"].nbytes > (3 << 19)                 # (past 1.5 sub-batches: the call is cut)
        assert _bad(f, _cyclic(eng, f["data"], logn, q, g, 0)) == []
        assert _bad(i, _cyclic(eng, i["data"], logn, q, g, 1)) == []
        fs = F.FourStep(eng, 1 << (logn // 2), 1 << (logn - logn // 2), q, g)
        src, dst = eng.upload(f["data"]), eng.alloc(f["data"].size)
        fs.ntt(src, dst, P)
        assert _bad(f, dst.download()) == []
        dst2 = eng.alloc(f["data"].size)
        flags = fs.ntt_checked(src, dst2, P)
        assert _bad(f, dst2.download()) == [] and flags.shape == (P,) and not flags.any()
        flags = fs.ntt_checked_phases(src, dst2, P)
        assert _bad(f, dst2.download()) == [] and flags.shape == (P, 3) and not flags.any()
        fs.close()


# ------------------------------------------------------------------ small and unusual moduli
@pytest.mark.parametrize("mod,root,logns", K.CASES, ids=[f"{m}-{r}" for m, r, _ in K.CASES])
def test_small_and_unusual_moduli(F, eng, O, mod, root, logns):
    """all mod - 1, alternating 0 / mod - 1, all mod // 2, a random vector and one with words at and above the modulus, against the
    oracle's cyclic transform (pinned to the plain-Python definition in tests/test_cyclic_small_moduli.py).  2^20 at 2^9 on the random
    vector is the input that showed the natural-order launches cannot serve roots that form no tower."""
    from fhe_reliability_gpu_amd._lib import FheError
    for logn in logns:
        N = 1 << logn
        for name, v in K.inputs(mod, logn):
            what = (mod, root, logn, name)
            assert F.ntt(v, mod, root) == O.ntt_cyclic(v, mod, root).tolist(), what
            assert F.intt(v, mod, root) == O.intt_cyclic(v, mod, root).tolist(), what
        names = [n for n, _ in K.inputs(mod, logn)]
        batch = np.stack([v for _, v in K.inputs(mod, logn)])
        n1 = 1 << (logn // 2)
        if logn >= 2 and (mod - 1) % N == 0 and K.has_tower(mod, root, logn):
            # the four-step's own reference (the direct DFT with w = root^((mod-1)/N)), which on these plans is the cyclic transform
            got = F.four_step_ntt(batch, N, mod, root, n1=n1)
            for name, v, y in zip(names, batch, got):
                assert y == O.ntt_cyclic(v, mod, root).tolist(), (mod, root, logn, name)
                if logn < 16 or name == "random":            # (two thirds of a second per vector at 2^16)
                    assert y == O.four_step_ntt(v, n1, N // n1, mod, root).tolist(), (mod, root, logn, name)
        elif logn >= 2:
            # N does not divide mod - 1, or root^((mod-1)/N) is no primitive root with w^(N/2) = -1 (998244353 with the quadratic
            # residue 4: there the reference's DFT and the network differ): the plan is refused with a status, not served wrongly
            with pytest.raises(FheError):
                F.four_step_ntt(batch, N, mod, root, n1=n1)
    eng.check()


@pytest.mark.parametrize("logn", [9, 13])
def test_forward_network_route_on_a_batch(eng, O, logn):
    """the route of the towerless calls at a single-launch and a two-launch size, a whole batch per call, forward and inverse (the
    scale rides on the bit-reversal gather): the even modulus 2^20, whose random vector showed the natural-order launches wrong"""
    mod, root = 1 << 20, 3
    batch = np.stack([v for _, v in K.inputs(mod, logn)] + [v for _, v in K.inputs(mod - 1, logn)])
    eng.trace(True)
    try:
        fwd = _cyclic(eng, batch, logn, mod, root, 0)
        inv = _cyclic(eng, batch, logn, mod, root, 1)
    finally:
        eng.trace(False)
    text = eng.trace_text()
    assert text.count("NTT_CYCLIC_FORWARD_NETWORK") == 2 and "NTT_CYCLIC_NATURAL_ORDER" not in text, text
    for v, a, b in zip(batch, fwd, inv):
        assert (a == O.ntt_cyclic(v, mod, root)).all() and (b == O.intt_cyclic(v, mod, root)).all()
    eng.check()


# ------------------------------------------------------------------ the two single-polynomial exports
@pytest.mark.parametrize("logn", [12, 16])
def test_inplace_exports_on_a_limb_window(F, eng, O, logn):
    """fhe_ntt_forward_inplace / fhe_ntt_inverse_inplace called directly: mixed 50 / 61-bit limbs, a window that does not start at
    limb 0, against the oracle's negacyclic transforms; windows outside the table set return a status and touch nothing."""
    from fhe_reliability_gpu_amd._lib import check, lib
    N = 1 << logn
    qs = F.create_moduli(N, [50, 61, 50, 61, 50])
    t = eng.tables(logn, qs)
    assert t.paths == [0, 1, 0, 1, 0]
    start, limbs = 1, 3
    rng = np.random.default_rng(logn)
    data = np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs[start:start + limbs]])
    data[0, :] = qs[start] - 1
    data[1, ::2] = qs[start + 1] - 1
    rps = [O.root_powers(q, logn) for q in qs[start:start + limbs]]
    fwd = np.stack([O.nwt_forward(data[l], qs[start + l], rps[l]) for l in range(limbs)])
    d = eng.upload(data)
    check(lib.fhe_ntt_forward_inplace(eng._h, d.ptr, t._h, limbs, start, None))
    assert (d.download() == fwd).all()
    check(lib.fhe_ntt_inverse_inplace(eng._h, d.ptr, t._h, limbs, start, None))
    assert (d.download() == data).all()
    check(lib.fhe_ntt_inverse_inplace(eng._h, d.ptr, t._h, limbs, start, None))      # and the inverse on words that are no image
    inv = np.stack([O.nwt_inverse(data[l], qs[start + l], rps[l]) for l in range(limbs)])
    assert (d.download() == inv).all()
    for f in (lib.fhe_ntt_forward_inplace, lib.fhe_ntt_inverse_inplace):
        assert f(eng._h, d.ptr, t._h, 3, 3, None) != 0          # runs past the last limb
        assert f(eng._h, d.ptr, t._h, 1, 5, None) != 0          # starts past it
        assert f(eng._h, d.ptr, None, 1, 0, None) != 0          # no tables
    assert (d.download() == inv).all()
    eng.check()
