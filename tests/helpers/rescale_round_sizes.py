"""What tests/test_gpu_rescale_round_sizes.py runs, apart from the definition (helpers/rescale_round.py): the table of shapes of each
of its sections, the functions that build their cases -- shared with tests/test_rescale_round_ref.py, which builds the same cases on the
CPU and holds the tile condition on them at 2^13 and 2^14 -- and the bodies of the sharded tests, which tests/test_gpu_rescale_round.py
calls at its own shapes."""
import numpy as np

from . import rescale_round as RR

U = np.uint64

# fhe_rescale, L = 3, K = 1: every two-launch size above 2^13 x both paths of the remaining limbs, an integer-path last limb over FP64
# limbs, and the 30-bit limbs under a 61-bit y at the sizes whose column plans differ most (2^15: Steps<4,3>; 2^17: rows of 512)
SIZES_RESCALE = [(logn, kind) for logn in (14, 15, 16, 17) for kind in ("50", "61+50last", "50+61last")] + [(15, "30+61last"), (17, "30+61last")]
# fhe_rescale, L = 5, K = 2: four runs of one limb each
SIZES_RUNS = [(13, "50/61/50/61/50"), (13, "61/50/61/50/61"), (14, "61/50/61/50/61"), (16, "50/61/50/61/50"), (16, "61/50/61/50/61")]
# fused fhe_hmult, K = 2, dnum 2: (logn, kind, L)
SIZES_HMULT = [(logn, kind, 3) for logn in (14, 15, 16, 17) for kind in ("50", "61", "50+61last")] + [(13, "50/61/50/61/50", 5), (15, "50/61/50/61/50", 5)]
# the plain route at N >= 2^13: (logn, option), each with the two prime sets below; L = 3, K = 2, dnum 2
SIZES_PLAIN = [(13, "ntt_resident"), (14, "ntt_resident"), (16, "ntt_mode")]
PLAIN_KINDS = ("50", "61+50last")


def case_seed(logn, kind):
    return 1000 * logn + 50 * (list(RR.PRIME_SETS) + list(RR.ALTERNATING)).index(kind)


def rescale_cases(qs, L, logn, seed, dictated=(1, 2, 3), fills=True):
    """the inputs of one fhe_rescale parametrisation at a two-launch size, [(name, parts, differs)]: dictated parts with the positions
    of every row class, y = h and y = h + 1 everywhere, and two random parts.  differs: whether nearest and floor differ at all -- not
    where y = h everywhere, whose centred remainder IS the remainder"""
    h = (int(qs[L - 1]) - 1) // 2
    cases = [(f"dictated, {n} parts", RR.dictated_parts(qs, L, logn, n, seed=seed + n, row_len=RR.ROW_LEN[logn]), True) for n in dictated]
    if fills:
        cases.append(("y = h everywhere", RR.dictated_parts(qs, L, logn, 1, seed=seed + 11, fill=h), False))
        cases.append(("y = h + 1 everywhere", RR.dictated_parts(qs, L, logn, 1, seed=seed + 12, fill=h + 1), True))
    cases.append(("random, 2 parts", RR.random_parts(qs, L, logn, 2, seed + 20), True))
    return cases


def runs_cases(qs, L, logn, seed):
    return rescale_cases(qs, L, logn, seed, dictated=(3,), fills=False)


def plain_cases(qs, L, logn, seed):
    return rescale_cases(qs, L, logn, seed, dictated=(2,), fills=False)


def plain_hmult_case(F, logn, kind):
    """the multiply of the plain-route section, and the moduli its rescale cases share"""
    return RR.hmult_case(F, logn, kind, 3, 2, 2, seed=case_seed(logn, kind) + 1)


def dictated_hmult_parts(qs, L, logn, seed=77):
    """(a0, a1) of a multiply by b = (1, 0) under a zero key: the relinearised product is (a0, a1) itself, so the fused route's y is
    the coefficient form of these parts' last limbs"""
    return RR.dictated_parts(qs, L, logn, 2, seed=seed, row_len=RR.ROW_LEN[logn])


# ------------------------------------------------------------------------------------------------ sharded phases (GPU; one process)
# shape of the second size the sharded bodies run at: rank 1's slab starts at clo = 3, a 61-bit limb under rank 0's 50-bit first limb
SHARD = dict(logn=15, bits=RR.limb_bits("50/61/50/61/50", 2), L=5, K=2, dnum=2)


def one_rank_parts(qs, L, logn, row_len=None):
    return np.stack([RR.dictated_parts(qs, L, logn, 1, seed=40 + i, row_len=row_len)[0] for i in range(2)])


def two_rank_inputs(qs, L, K, dnum, logn, row_len=None):
    """(a0, a1, b0, b1, key) of the multiply and the three parts of the rescale"""
    N = 1 << logn
    rng = np.random.default_rng(5)
    rnd = lambda qq: np.stack([rng.integers(0, q, N, dtype=U) for q in qq])
    a0, a1, b0, b1 = (rnd(qs[:L]) for _ in range(4))
    key = np.stack([np.stack([rnd(qs) for _ in range(2)]) for _ in range(dnum)])
    return (a0, a1, b0, b1, key), RR.dictated_parts(qs, L, logn, 3, seed=9, row_len=row_len)


def to_cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def from_cuda(t):
    return t.cpu().numpy().view(U)


def one_rank_phase_path(F, eng, logn, bits, L, K, dnum, row_len=None, floor_again=False):
    """a sharded plan of world 1: fhe_rescale_shard_begin / _finish give the single call's words, and those are the reference's, whose
    every tile tells nearest from floor.  floor_again: then mode 0 on the same two plans, against the flooring oracle"""
    import torch

    from fhe_reliability_gpu_amd.dist import ShardedKeySwitch
    N = 1 << logn
    qs = F.create_moduli(N, bits)
    t = eng.tables(logn, qs)
    parts = one_rank_parts(qs, L, logn, row_len)
    want, floor = RR.references(parts, qs, L, logn, True, "one rank")
    ks = F.KeySwitch(eng, t, L, K, dnum)
    ks.set_rescale_rounding(True)
    RR.same(ks.rescale(eng.upload(parts), 2), want, "single call")
    sh = ShardedKeySwitch(eng, t, L, K, dnum)
    sh.set_rescale_rounding(True)
    assert sh.rescale_rounding is True
    loc = to_cuda(parts)

    def phases():
        torch.cuda.synchronize()
        with sh.stream_scope():
            sh.rescale_begin(loc)
            out = sh.rescale_finish(loc)
        torch.cuda.synchronize()
        return from_cuda(out)

    assert (phases() == want).all()
    if floor_again:
        ks.set_rescale_rounding(False)
        sh.set_rescale_rounding(False)
        assert sh.rescale_rounding is False
        RR.same(ks.rescale(eng.upload(parts), 2), floor, "single call, floor after nearest")
        got = phases()
        assert (got == floor).all(), f"phases, floor after nearest: {int((got != floor).sum())} words differ"


def two_ranks_in_one_process(F, eng, logn, bits, L, K, dnum, row_len=None, floor_again=False):
    """both ranks' plans in one process, the host doing the collectives: fhe_rescale_shard_* against the reference, whose every tile
    tells nearest from floor, and the fused multiply's finish, gathered limbs against the single-device words.  floor_again: the
    multiply's words are held against the reference here as well (tile condition included), and both are run once more in mode 0 on the
    same plans, against the flooring oracle"""
    import ctypes as C

    import torch

    from fhe_reliability_gpu_amd._lib import check, lib, vp
    from fhe_reliability_gpu_amd.dist import ks_layout, own_ct_rows, own_rows
    world = 2
    N = 1 << logn
    qs = F.create_moduli(N, bits)
    t = eng.tables(logn, qs)
    (a0, a1, b0, b1, key), parts = two_rank_inputs(qs, L, K, dnum, logn, row_len)
    P = lambda x: C.c_void_p(x.data_ptr() if x is not None and x.numel() else 0)
    lays = [ks_layout(L, K, world, r) for r in range(world)]
    cmax, smax = lays[0]["cmax"], lays[0]["smax"]
    zeros = lambda rows: torch.zeros((rows, N), dtype=torch.int64, device="cuda")
    g1, g2, bc = [zeros(world * cmax) for _ in range(world)], [zeros(world * 2 * smax) for _ in range(world)], [zeros(3) for _ in range(world)]
    plans = []
    for r in range(world):
        h = vp()
        check(lib.fhe_keyswitch_create_sharded(eng._h, t._h, L, K, dnum, world, r, P(g1[r]), P(g2[r]), P(bc[r]), C.byref(h)))
        check(lib.fhe_keyswitch_set_rescale_rounding(h, 1))
        plans.append(h)
    owner = next(r for r, l in enumerate(lays) if l["clo"] <= L - 1 < l["clo"] + l["cn"])
    rs_rows = [max(0, min(l["clo"] + l["cn"], L - 1) - l["clo"]) for l in lays]
    empty = lambda *shape: torch.empty(shape, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def gather(bufs, rows):
        torch.cuda.synchronize()
        for r in range(world):
            for s in range(world):
                if r != s:
                    bufs[r][s * rows:(s + 1) * rows] = bufs[s][s * rows:(s + 1) * rows]
        torch.cuda.synchronize()

    def bcast(n_rows):
        torch.cuda.synchronize()
        for r in range(world):
            if r != owner:
                bc[r][:n_rows] = bc[owner][:n_rows]
        torch.cuda.synchronize()

    pl = [to_cuda(parts[:, own_ct_rows(lays[r])]) for r in range(world)]
    loc = lambda a, r: to_cuda(a[own_ct_rows(lays[r])])
    keyl = [to_cuda(key[:, :, own_rows(lays[r])]) for r in range(world)]
    ops = [[loc(v, r) for v in (a0, a1, b0, b1)] for r in range(world)]

    def rescale_phases():
        for r in range(world):
            check(lib.fhe_rescale_shard_begin(eng._h, plans[r], P(pl[r]), 3, None))
        bcast(3)
        outs = []
        for r in range(world):
            o = empty(3, rs_rows[r], N)
            check(lib.fhe_rescale_shard_finish(eng._h, plans[r], P(o), P(pl[r]), 3, None))
            outs.append(o)
        eng.sync()
        return np.concatenate([from_cuda(o) for o in outs], axis=1)

    def hmult_phases():
        d = []
        for r in range(world):
            x = ops[r]
            dd = [torch.empty_like(x[0]) for _ in range(3)]
            check(lib.fhe_tensor_product(eng._h, P(dd[0]), P(dd[1]), P(dd[2]), P(x[0]), P(x[1]), P(x[2]), P(x[3]), t._h, lays[r]["cn"], lays[r]["clo"], None))
            d.append(dd)
        for r in range(world):
            check(lib.fhe_keyswitch_shard_begin(eng._h, plans[r], P(d[r][2]), None))
        gather(g1, cmax)
        for r in range(world):
            check(lib.fhe_keyswitch_shard_inner(eng._h, plans[r], P(d[r][2]), P(keyl[r]), None))
        gather(g2, 2 * smax)
        for r in range(world):
            check(lib.fhe_hmult_shard_finish_begin(eng._h, plans[r], P(d[r][0]), P(d[r][1]), None))
        bcast(2)
        outs = []
        for r in range(world):
            o = empty(2, rs_rows[r], N)
            check(lib.fhe_hmult_shard_finish_end(eng._h, plans[r], P(o[0]), P(o[1]), P(d[r][0]), P(d[r][1]), None))
            outs.append(o)
        eng.sync()
        return np.stack([np.concatenate([from_cuda(o[i]) for o in outs]) for i in range(2)])

    try:
        # ---- the rescale of three parts
        want, floor = RR.references(parts, qs, L, logn, True, "two ranks, rescale")
        assert (rescale_phases() == want).all()
        # ---- the fused multiply's finish
        assert lib.fhe_hmult_shard_fusable(eng._h, plans[0])
        ks = F.KeySwitch(eng, t, L, K, dnum)
        ks.set_rescale_rounding(True)
        up = [eng.upload(x) for x in (a0, a1, b0, b1, key)]
        h0, h1 = ks.hmult(*up, rescale=True)
        hw = np.stack([h0.download().reshape(L - 1, N), h1.download().reshape(L - 1, N)])
        if floor_again:
            hnear, hfloor = RR.references(RR.hmult_relin_ref(qs, a0, a1, b0, b1, key, L, K, dnum, logn), qs, L, logn, True, "two ranks, multiply")
            assert (hw == hnear).all()
        got = hmult_phases()
        assert (got[0] == hw[0]).all()
        assert (got[1] == hw[1]).all()
        if floor_again:
            # ---- mode 0 on the same plans
            for p in plans:
                check(lib.fhe_keyswitch_set_rescale_rounding(p, 0))
            got = rescale_phases()
            assert (got == floor).all(), f"rescale, floor after nearest: {int((got != floor).sum())} words differ"
            ks.set_rescale_rounding(False)
            f0, f1 = ks.hmult(*up, rescale=True)
            RR.same(f0, hfloor[0], "single device, floor after nearest, part 0")
            RR.same(f1, hfloor[1], "single device, floor after nearest, part 1")
            got = hmult_phases()
            assert (got == hfloor).all(), f"fused finish, floor after nearest: {int((got != hfloor).sum())} words differ"
    finally:
        for h in plans:
            lib.fhe_keyswitch_destroy(h)
    return lays
