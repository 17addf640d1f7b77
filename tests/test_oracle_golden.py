"""Pin the CPU oracle (oracle/) against the golden vectors produced by the
reference's own Python (tests/golden/make_golden.py) and against the data files the
reference holds.  CPU only."""
import random

import numpy as np

from conftest import load_golden, sha_u64
from oracle import cport as C
from oracle import pyport as P

Q61 = 2305843009211596801
PHANTOM_PRIMES = [1125899903107073, 1125899903500289, 1125899903795201,
                  1125899903827969, 1125899903991809, 1125899904679937]


# ------------------------------------------------------------------ a10
def test_prime_rule_matches_logged_phantom_primes():
    # reliability_test/data/bits1-16_num1.txt:10
    assert C.gen_primes(16384, 50, 6) == PHANTOM_PRIMES
    assert P.gen_primes(16384, 50, 6) == PHANTOM_PRIMES


def test_min_root_and_tables_kat2():
    q, logn = PHANTOM_PRIMES[0], 14
    psi = C.min_primitive_root(q, 2 << logn)
    assert psi == 32853495844 == P.min_primitive_root(q, 2 << logn)
    rp, sh = C.root_powers(q, logn, psi, shoup=True)
    assert int(rp[1]) == 163343304402113 and int(sh[1]) == 2676216708203466951
    a = np.array([(i * i + 1) % q for i in range(1 << logn)], dtype=np.uint64)
    out = C.nwt_forward(a, q, rp)
    assert [int(x) for x in out[:4]] == [1037891225979181, 928784233542420, 626683383818997, 933202470215772]
    assert sha_u64(out) == "79d3fd044499dd0c43406c0e0d282a73b2aba27be4fdb7efba6342e00d9a3a4d"
    assert (C.nwt_inverse(out, q, rp) == a).all()


def test_kat1_hand_checkable():
    rp = P.root_powers(17, 3, 3)
    assert rp == [1, 13, 9, 15, 3, 5, 10, 11]
    assert P.nwt_forward(list(range(1, 9)), 17, rp) == [5, 0, 13, 8, 9, 11, 5, 8]
    assert list(C.nwt_forward(np.arange(1, 9), 17, rp)) == [5, 0, 13, 8, 9, 11, 5, 8]


# ------------------------------------------------------------------- a1
def test_cyclic_ntt_against_reference_vectors():
    g = load_golden("cyclic_ntt.json")
    d = g["demo"]
    assert list(C.ntt_cyclic(d["a"], d["mod"], d["root"])) == d["A"]
    assert P.ntt_cyclic(d["a"], d["mod"], d["root"]) == d["A"]
    for case in g["cases"]:
        random.seed(case["seed"])
        a = [random.randrange(case["mod"]) for _ in range(1 << case["lg"])]
        if "a" in case:
            assert a == case["a"]
        out = C.ntt_cyclic(a, case["mod"], case["root"])
        assert sha_u64(out) == case["sha256"]
        assert [int(x) for x in out[:8]] == case["head"] and [int(x) for x in out[-8:]] == case["tail"]
        if case["lg"] <= 10:
            assert P.ntt_cyclic(a, case["mod"], case["root"]) == case["out"]
    t = g["bsgs_twin"]
    assert list(C.ntt_cyclic(t["a"], t["mod"], t["root"])) == t["fwd"]
    assert list(C.intt_cyclic(t["fwd"], t["mod"], t["root"])) == t["inv_of_fwd"] == t["a"]
    assert P.intt_cyclic(t["fwd"], t["mod"], t["root"]) == t["a"]
    r = g["rfhe_twin"]
    assert list(C.ntt_cyclic(r["a"], r["mod"], r["root"])) == r["fwd"]
    assert list(C.intt_cyclic(r["a"], r["mod"], r["root"])) == r["inv"]
    r = g["nthroot"]
    assert list(C.ntt_nthroot(r["a"], r["root"], r["mod"])) == r["fwd"] == P.ntt_nthroot(r["a"], r["root"], r["mod"])
    assert P.intt_nthroot(r["a"], r["root"], r["mod"]) == r["inv"]


def test_survey_known_answers_cyclic():
    # SURVEY section 8c fixtures
    random.seed(12)
    a = [random.randrange(Q61) for _ in range(1 << 12)]
    out = C.ntt_cyclic(a, Q61, 37)
    assert sha_u64(out) == "d450c57eb5357e3437cc9f21ba81d93b496109d989b5e4d5c904051ba22e9ee2"


# -------------------------------------------------------------- a2/a3/a5
def test_negacyclic_against_reference_vectors():
    g = load_golden("negacyclic.json")
    for case in g["cases"]:
        n, q, psi = case["n"], case["q"], case["psi"]
        random.seed(case["seed"])
        a = [random.randrange(q) for _ in range(n)]
        fwd = C.negacyclic_ntt(a, psi, q)
        assert sha_u64(fwd) == case["sha256_fwd"]
        assert [int(x) for x in fwd[:8]] == case["head"]
        assert (C.negacyclic_intt(fwd, psi, q) == np.array(a, dtype=np.uint64)).all()
        # Phantom ordering == reference natural-order output read at bit-reversed indices (A4)
        logn = n.bit_length() - 1
        rp = C.root_powers(q, logn, psi)
        nwt = C.nwt_forward(a, q, rp)
        idx = np.array([P.bit_reverse(i, logn) for i in range(n)])
        assert (nwt == fwd[idx]).all()
        assert (C.nwt_inverse(nwt, q, rp) == np.array(a, dtype=np.uint64)).all()
        if n <= 64:
            assert P.negacyclic_ntt(a, psi, q) == case["fwd"]
            assert P.nwt_forward(a, q, P.root_powers(q, logn, psi)) == [int(x) for x in nwt]
    for pm in g["polymul"]:
        c = C.polymul_ntt(pm["a"], pm["b"], pm["psi"], pm["q"])
        assert list(c) == pm["c"]
        assert list(C.polymul_naive(pm["a"], pm["b"], pm["q"])) == pm["c"]
        if pm["n"] <= 32:
            assert P.poly_mul_negacyclic_ntt(pm["a"], pm["b"], pm["psi"], pm["q"]) == pm["c"]


def test_minimal_psi_is_a_power_of_logged_root():
    # the sub-ring roots used in the golden file are powers of the N=16384 root; the
    # engine always takes the MINIMAL root, so check both give valid transforms
    q = PHANTOM_PRIMES[0]
    for logn in (3, 6, 10):
        psi = C.min_primitive_root(q, 2 << logn)
        assert pow(psi, 1 << logn, q) == q - 1


# ------------------------------------------------------------------- a6
def test_four_step_against_reference_vectors():
    g = load_golden("four_step.json")
    for case in g["cases"]:
        N = case["N"]
        n1 = int(round(N ** 0.5))
        assert list(C.four_step_ntt(case["a"], n1, n1, g["mod"], g["g"])) == case["y"]
        assert list(C.ntt_direct(case["a"], g["mod"], g["g"])) == case["y"]
        if N <= 64:
            assert P.four_step_ntt(case["a"], n1, n1, g["mod"], g["g"]) == case["y"]
    # generalisation n1 != n2: equals the direct transform and motivation's cyclic NTT
    random.seed(1)
    a = [random.randrange(g["mod"]) for _ in range(128)]
    d = C.ntt_direct(a, g["mod"], g["g"])
    assert (C.four_step_ntt(a, 16, 8, g["mod"], g["g"]) == d).all()
    assert (C.four_step_ntt(a, 8, 16, g["mod"], g["g"]) == d).all()
    assert (C.ntt_cyclic(a, g["mod"], g["g"]) == d).all()


# ------------------------------------------------------------------- a7
def test_barrett_matches_exact_remainder():
    rng = random.Random(3)
    for q in (PHANTOM_PRIMES[0], Q61, 137438953481, 17, (1 << 62) - 57):
        K, mu = C.barrett_ctx(q)
        assert (K, mu) == P.barrett_ctx(q)
        for _ in range(200):
            a, b = rng.randrange(q), rng.randrange(q)
            t = a * b
            assert C.barrett_reduce(t, q, K, mu) == t % q == P.barrett_reduce(t, q, K, mu)
        for t in (0, q - 1, q, q * q - 1, (q - 1) * (q - 1)):
            assert C.barrett_reduce(t, q, K, mu) == t % q


# ------------------------------------------------------------------- a8
def test_base_conversion_against_reference_vectors():
    g = load_golden("baseconv.json")
    for key in ("exact", "exact50"):
        e = g[key]
        out = C.baseconv_exact(e["res"], e["mod_in"], e["mod_out"])
        assert out.tolist() == e["out"]
        assert P.base_conv_fixed(e["res"], e["mod_in"], e["mod_out"]) == e["out"]
    for key in ("fast", "fast31"):
        f = g[key]
        out = C.bconv_fast(f["res"], f["mod_in"], f["mod_out"])
        assert out.tolist() == f["out"]
        assert P.bconv_fast(f["res"], f["mod_in"], f["mod_out"]) == f["out"]


def test_crt_garner_roundtrip_and_reference_build():
    # property asserted by the reference at rfhe_framewk/src/baseConv.cu:200-205
    rng = random.Random(11)
    # 4 limbs x 20 bits as in the reference's main (baseConv.cpp:176-178); its
    # crt_reconstruct overflows u128 once P * p_j exceeds 128 bits
    mod = [1048583, 1048589, 1048601, 1048609]
    assert all(P.is_prime(p) for p in mod)
    N = 64
    res = [[rng.randrange(p) for _ in range(N)] for p in mod]
    lo, hi = C.crt_garner(res, mod)
    py = P.crt_garner(res, mod)
    for i in range(N):
        x = (int(hi[i]) << 64) | int(lo[i])
        assert (int(lo[i]), int(hi[i])) == py[i]
        for j, p in enumerate(mod):
            assert x % p == res[j][i]
    # same integers as the reference's own crt_reconstruct: its recorded outputs (tests/golden/crt_reconstruct.json,
    # make_golden.py dump_crt) always, and the live oracle/_ref build as well where `make -C oracle ref` made one
    g = load_golden("crt_reconstruct.json")
    assert g["mod"] == mod and g["res"] == res
    assert lo.tolist() == g["lo"] and hi.tolist() == g["hi"]
    ref = C.ref_crt_reconstruct(res, mod)
    if ref is not None:
        assert (ref[0] == lo).all() and (ref[1] == hi).all()


# ------------------------------------------------------------------- a9
def test_bsgs_hadamard_against_reference_vectors():
    g = load_golden("bsgs.json")
    s = g["small"]
    assert C.bsgs_hadamard(s["M"], s["v"]).tolist() == s["y"]
    assert P.diag_block_hadamard_matvec(s["M"], s["v"]) == s["y"]
    # the module-level workload of motivation/bsgs.py:89-101 (np.random.seed(0))
    np.random.seed(g["numpy_seed"])
    M = [np.random.randint(0, g["mod"], size=g["block_size"]) for _ in range(g["k"])]
    v = np.random.randint(0, g["mod"], size=g["block_size"] * g["k"])
    assert sha_u64([int(x) for b in M for x in b]) == g["sha256_M"]
    y = C.bsgs_hadamard(np.array(M), v)
    assert y[:32].tolist() == g["y_head"]
    assert sha_u64(y.astype(np.uint64)) == g["sha256_y"]
