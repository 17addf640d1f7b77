"""The reference's bit-flip experiment with a detector verdict next to its corruption count.

reliability_test/dotprod_test.cu:31-61 flips ``bits_per_symbol`` bits in each of ``num_symbols`` words of an encrypted operand in
memory, then runs multiply -> relinearize -> mod_switch (:113-115) and log2(row) rounds of rotate + add (:143-148).  Here the same
chain runs on a BGV plan of the same shape (default N = 2^14, six 50-bit primes of which two are special, plain modulus 65537,
:199-204) through the sealed calls: the operands and keys are sealed, one operand is flipped at rest with ``fhe_flip_bit``, then
    hmult_sealed (rescale)  ->  log2(row) x [ rotate_sealed  ->  seal_verify of both summands, modadd_checked, seal of the sum ]
and per trial the tool prints how many words of the final ciphertext differ from the clean run's, how many flag words were raised
anywhere in the chain, and whether the fault was detected.  The operands are uniformly random residues, not encryptions: the tool
measures detection, it decrypts nothing.  Unlike the reference, the bits flipped in one word are distinct, so that every trial with
a flip changes memory.  Trial 0 flips nothing (control).  The product has L - 1 limbs, so the rotation rounds run on a second plan
over the remaining primes.  Exit status 1 when a trial with at least one flip was not detected.

--repair runs the same experiment through the repairing composites (hmult_sealed_repair, rotate_sealed_repair): operands and keys
carry locators beside their seals, and per trial the tool prints how many rows were corrected, how many were left uncorrectable or
suspect, whether the trial was missed (a flip, no repair and no flag), and whether the final words equal the fault-free run's bit for
bit.  One flipped word per row is corrected and the chain then computes the clean result; two or more symbols in one row stay
uncorrectable, as the flags say.  Exit status 1 when a trial was missed, or was reported all corrected with a final result that differs.

--rotate-sum runs the reference's whole experiment, its tail included, through two protected calls: hmult_sealed, then
rotate_sum_sealed, whose carried adds verify their operands on the load that feeds the adder and hand the seals on without a sealing
or verifying launch in between.  Output and exit status as in the default mode; the fault-free words equal the default chain's.

--bsgs applies the same fault model to the operands a linear layer keeps longest: a CKKS plan of the same shape runs
bsgs_matvec_sealed (n1 = n2 = 4) with every operand sealed, and each trial flips its bits in a diagonal (odd trials) or in a giant key
(even trials) at rest.  Per trial the tool prints which flag groups were raised; a diagonal is caught by the inner sum itself, on
the load that multiplies it.  Exit status as in the default mode.

--fused runs the default chain (or, with --rotate-sum, that one) with hmult_sealed_fused in the place of hmult_sealed: the four operand
sweeps are gone and the flipped operand is caught by the tensor step itself, on the load that multiplies it.  The fault-free words
are held against the sweep-based chain's first.  Output and exit status as in the default mode.

--fused-key applies the same fault model to the relinearisation key at rest, the largest and longest-lived operand of the multiply,
and runs hmult_sealed_fused_key: no input is swept at all, and the flipped key word is caught by the key switch's inner product
itself, on the load that multiplies it.  The fault-free words and flags are held against hmult_sealed's first.  Per trial the tool
prints which key rows were raised.  Exit status as in the default mode.

--ntt runs the reference's other experiment, reliability_test/ntt_test.cu:104-144, with a verdict: a batch of ``--batch`` random rows
(one 50-bit prime each, as ``ntt_test <log_dim> <batch_size>``) is sealed, each trial places its flips in the source of the forward
transform at rest, and ntt_sealed must raise exactly the flipped rows in its input block, raise nothing in its ABFT block, and leave
exactly those rows with a poisoned output seal, which a seal_verify sweep of the result then refuses.  Per trial the tool prints
the reference's damage count (output words that differ, the symbol error rate) next to the rows raised.  The control trial must
raise nothing and produce seals equal to seal(dst).  Exit status 1 when a trial's raised rows are not its flipped rows.

--polymul applies the same fault model to the factors of the negacyclic product at rest (the protected chain of
rfhe_framewk/src/four_step_ntt_protected.py:219-282): two batches of ``--batch`` random rows are sealed, each trial places its flips in
a or b at rest, and polymul_sealed must raise exactly the flipped rows in exactly the flipped factor's block, raise nothing in the
checked product's own block -- the corrupted factor is a consistent input to all three ABFT identities -- and leave exactly those
rows with a poisoned output seal.  The control trial must raise nothing and produce seals equal to seal(c).  Exit status as --ntt.

python -m fhe_reliability_gpu_amd.tools.flip_coverage [--repair | --rotate-sum | --bsgs | --fused | --fused-key | --ntt [--batch 4] | --polymul [--batch 4]] [--trials 32] [--num-symbols 1] [--bits-per-symbol 1] [--logn 14] [--row 8] [--seed 1]"""
import argparse
import sys

import numpy as np

import fhe_reliability_gpu_amd as F
from fhe_reliability_gpu_amd._lib import check, lib

PLAIN_MODULUS = 65537
L, K, DNUM = 4, 2, 2


def nonzero(flags):
    """raised flag words of a (nested) flag dictionary or array"""
    if flags is None:
        return 0
    if isinstance(flags, dict):
        return sum(nonzero(v) for v in flags.values())
    if isinstance(flags, (list, tuple)):
        return sum(nonzero(v) for v in flags)
    return int(np.count_nonzero(flags))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--trials", type=int, default=32)
    ap.add_argument("--num-symbols", type=int, default=1)
    ap.add_argument("--bits-per-symbol", type=int, default=1)
    ap.add_argument("--logn", type=int, default=14)
    ap.add_argument("--row", type=int, default=8, help="slots summed by the rotate-and-add rounds (a power of two)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--repair", action="store_true", help="run the chain through the repairing composites and report corrections")
    ap.add_argument("--rotate-sum", action="store_true", help="run the rotate-and-add rounds as one rotate_sum_sealed call")
    ap.add_argument("--bsgs", action="store_true", help="flip a diagonal or a giant key of a sealed BSGS matrix-vector product")
    ap.add_argument("--fused", action="store_true", help="run the multiply as hmult_sealed_fused: operands verified on the multiplying load")
    ap.add_argument("--fused-key", action="store_true", help="flip the relinearisation key at rest and run hmult_sealed_fused_key")
    ap.add_argument("--ntt", action="store_true", help="flip the source of the forward transform at rest and run ntt_sealed (ntt_test.cu:104-144)")
    ap.add_argument("--polymul", action="store_true", help="flip a factor of the negacyclic product at rest and run polymul_sealed")
    ap.add_argument("--batch", type=int, default=4, help="--ntt, --polymul: rows of the batch, one 50-bit prime each")
    a = ap.parse_args()
    if a.polymul and (a.ntt or a.repair or a.bsgs or a.rotate_sum or a.fused or a.fused_key):
        ap.error("--polymul is a mode of its own")
    if a.ntt and (a.repair or a.bsgs or a.rotate_sum or a.fused or a.fused_key):
        ap.error("--ntt is a mode of its own")
    if a.fused_key and (a.repair or a.bsgs or a.rotate_sum or a.fused):
        ap.error("--fused-key is a mode of its own")
    if a.fused and (a.repair or a.bsgs):
        ap.error("--fused goes with the default chain or with --rotate-sum: the fused multiply has no repairing form")
    if a.repair and a.rotate_sum:
        ap.error("--repair and --rotate-sum exclude each other: the composite has no repairing form")
    if a.bsgs and (a.repair or a.rotate_sum):
        ap.error("--bsgs is a mode of its own")
    if a.row < 1 or a.row & (a.row - 1) or not 1 <= a.bits_per_symbol <= 64 or a.num_symbols < 0:
        ap.error("row is a power of two, bits-per-symbol 1..64, num-symbols >= 0")
    eng = F.Engine(0)
    if a.ntt:
        return main_ntt(a, eng)
    if a.polymul:
        return main_polymul(a, eng)
    if a.bsgs:
        return main_bsgs(a, eng)
    if a.fused_key:
        return main_fused_key(a, eng)
    N, R = 1 << a.logn, L - 1
    qs = F.create_moduli(N, [50] * (L + K))
    rng = np.random.default_rng(a.seed)
    t = eng.tables(a.logn, qs)
    ks, ab = F.KeySwitch(eng, t, L, K, DNUM), F.Abft(eng, t)
    ks.set_plain_modulus(PLAIN_MODULUS)
    # the level below: the product's primes and the special ones
    qs2 = qs[:R] + qs[L:]
    t2 = eng.tables(a.logn, qs2)
    ks2, ab2 = F.KeySwitch(eng, t2, R, K, DNUM), F.Abft(eng, t2)
    ks2.set_plain_modulus(PLAIN_MODULUS)
    poly = lambda moduli: np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in moduli])
    key = lambda moduli: np.stack([np.stack([poly(moduli) for _ in range(2)]) for _ in range(DNUM)])
    ct_a, ct_b = np.stack([poly(qs[:L]), poly(qs[:L])]), np.stack([poly(qs[:L]), poly(qs[:L])])
    rounds = a.row.bit_length() - 1
    elts = [pow(5, 1 << r, 2 * N) for r in range(rounds)]
    d_b, d_rlk = eng.upload(ct_b), eng.upload(key(qs))
    d_gk = [eng.upload(key(qs2)) for _ in elts]
    # seals, taken once of the clean data: what travels with the ciphertexts and keys
    s_b = t.seal(d_b, limbs=L, n_poly=2)
    s_rlk, s_gk = ks.seal_key(d_rlk), [ks2.seal_key(g) for g in d_gk]
    s_a = t.seal(eng.upload(ct_a), limbs=L, n_poly=2)
    if a.repair:      # the locators that travel with the seals
        l_b, l_a = t.seal_locator(d_b, limbs=L, n_poly=2), t.seal_locator(eng.upload(ct_a), limbs=L, n_poly=2)
        l_rlk, l_gk = ks.seal_key_locator(d_rlk), [ks2.seal_key_locator(g) for g in d_gk]
    part = lambda d, i, limbs: _view(eng, d, i * limbs * N, limbs * N)
    seal_part = lambda s, i, limbs: _view(eng, s, i * limbs * 2, limbs * 2)

    hmult = ks.hmult_sealed

    def chain(d_a):
        """the sealed chain on operand d_a (sealed as s_a); returns the final parts and the raised flag words"""
        raised = 0
        o0, o1, so, fl = hmult(part(d_a, 0, L), part(d_a, 1, L), part(d_b, 0, L), part(d_b, 1, L), d_rlk, ab,
                                         seals=[seal_part(s_a, 0, L), seal_part(s_a, 1, L), seal_part(s_b, 0, L), seal_part(s_b, 1, L)], key_seal=s_rlk)
        raised += nonzero(fl)
        c, sc = [o0, o1], list(so)
        for elt, gk, sgk in zip(elts, d_gk, s_gk):
            r0, r1, sr, fl = ks2.rotate_sealed(c[0], c[1], elt, gk, ab2, seals=sc, key_seal=sgk)
            raised += nonzero(fl)
            for h, (rot, srot) in enumerate(((r0, sr[0]), (r1, sr[1]))):
                raised += nonzero(t2.seal_verify(c[h], sc[h], limbs=R)) + nonzero(t2.seal_verify(rot, srot, limbs=R))
                raised += nonzero(t2.modadd_checked(c[h], c[h], rot, limbs=R))
                sc[h] = t2.seal(c[h], limbs=R)
        return np.concatenate([c[0].download().reshape(-1), c[1].download().reshape(-1)]), raised

    def chain_sum(d_a):
        """the same chain with its tail as one call: hmult_sealed, then rotate_sum_sealed on its outputs and their seals"""
        o0, o1, so, fl = hmult(part(d_a, 0, L), part(d_a, 1, L), part(d_b, 0, L), part(d_b, 1, L), d_rlk, ab,
                                         seals=[seal_part(s_a, 0, L), seal_part(s_a, 1, L), seal_part(s_b, 0, L), seal_part(s_b, 1, L)], key_seal=s_rlk)
        raised = nonzero(fl)
        if elts:
            o0, o1, so, steps = ks2.rotate_sum_sealed(o0, o1, elts, d_gk, ab2, so, key_seals=s_gk)
            raised += sum(nonzero(st) for st in steps)
        # the seals the chain hands on are those of the words it hands on, unless a flag says otherwise
        raised += nonzero(t2.seal_verify(o0, so[0], limbs=R)) + nonzero(t2.seal_verify(o1, so[1], limbs=R))
        return np.concatenate([o0.download().reshape(-1), o1.download().reshape(-1)]), raised

    def outcomes(reports, tally):
        for rep in reports.values():
            for status in np.asarray(rep).reshape(-1, 4)[:, 0].tolist():
                tally[int(status)] = tally.get(int(status), 0) + 1

    def chain_repair(d_a):
        """the same chain through the repairing composites; returns the final parts, the raised flag words and the outcome tally"""
        raised, tally = 0, {}
        loc_part = lambda s, i, limbs: _view(eng, s, i * limbs, limbs)
        o0, o1, so, lo, fl, rep = ks.hmult_sealed_repair(
            part(d_a, 0, L), part(d_a, 1, L), part(d_b, 0, L), part(d_b, 1, L), d_rlk, ab,
            seals=[seal_part(s_a, 0, L), seal_part(s_a, 1, L), seal_part(s_b, 0, L), seal_part(s_b, 1, L)],
            locators=[loc_part(l_a, 0, L), loc_part(l_a, 1, L), loc_part(l_b, 0, L), loc_part(l_b, 1, L)], key_seal=s_rlk, key_locator=l_rlk)
        raised += nonzero(fl)
        outcomes(rep, tally)
        c, sc, lc = [o0, o1], list(so), list(lo)
        for elt, gk, sgk, lgk in zip(elts, d_gk, s_gk, l_gk):
            r0, r1, sr, lr, fl, rep = ks2.rotate_sealed_repair(c[0], c[1], elt, gk, ab2, seals=sc, locators=lc, key_seal=sgk, key_locator=lgk)
            raised += nonzero(fl)
            outcomes(rep, tally)
            for h, (rot, srot, lrot) in enumerate(((r0, sr[0], lr[0]), (r1, sr[1], lr[1]))):
                for words, seal, loc in ((c[h], sc[h], lc[h]), (rot, srot, lrot)):
                    f, rp = t2.seal_repair(words, seal, loc, limbs=R)
                    raised += nonzero(f)
                    outcomes({"rows": rp}, tally)
                raised += nonzero(t2.modadd_checked(c[h], c[h], rot, limbs=R))
                sc[h], lc[h] = t2.seal(c[h], limbs=R), t2.seal_locator(c[h], limbs=R)
        return np.concatenate([c[0].download().reshape(-1), c[1].download().reshape(-1)]), raised, tally

    clean, raised = chain(eng.upload(ct_a))
    assert raised == 0, "the clean chain raised a flag"
    if a.fused:
        hmult = ks.hmult_sealed_fused
        out, raised = chain(eng.upload(ct_a))
        assert raised == 0 and (out == clean).all(), "the clean chain with the fused multiply differs from the sealed chain"
    if a.repair:
        return main_repair(a, eng, rng, ct_a, clean, chain_repair)
    if a.rotate_sum:
        out, raised = chain_sum(eng.upload(ct_a))
        assert raised == 0 and (out == clean).all(), "the clean rotate-and-sum chain differs from the sealed chain"
        chain = chain_sum
    print(f"N = 2^{a.logn}, L = {L}, K = {K}, dnum = {DNUM}, plain modulus {PLAIN_MODULUS}; {rounds} rotate-and-add rounds"
          f"{' as one rotate_sum_sealed call' if a.rotate_sum else ''}{'; multiply: hmult_sealed_fused' if a.fused else ''}; {a.num_symbols} symbols x {a.bits_per_symbol} bits per trial")
    missed = 0
    for trial in range(a.trials):
        d_a = eng.upload(ct_a)
        n_sym = 0 if trial == 0 else a.num_symbols
        for idx in rng.integers(0, ct_a.size, n_sym):
            for bit in rng.choice(64, a.bits_per_symbol, replace=False):
                check(lib.fhe_flip_bit(eng._h, d_a.ptr, int(idx), int(bit), None))
        flipped = int(np.count_nonzero(d_a.download().reshape(-1) != ct_a.reshape(-1)))
        out, raised = chain(d_a)
        corrupted = int(np.count_nonzero(out != clean))
        detected = raised > 0
        missed += flipped > 0 and not detected
        assert flipped > 0 or (corrupted == 0 and not detected), "the control trial differs from the clean run"
        print(f"trial {trial:3d}: flipped words {flipped:3d}, corrupted output words {corrupted:7d} of {out.size}, raised flag words {raised:4d}, "
              f"detected {'yes' if detected else 'no'}", flush=True)
    eng.check()
    print(f"summary: {a.trials} trials, {missed} with a flip and no flag")
    return 1 if missed else 0


def main_repair(a, eng, rng, ct_a, clean, chain_repair):
    """the trials of --repair: the same flips, the chain through the repairing composites"""
    out, raised, tally = chain_repair(eng.upload(ct_a))
    assert raised == 0 and (out == clean).all() and set(tally) <= {F.SEAL_CLEAN}, "the clean repairing chain differs from the sealed chain"
    print(f"N = 2^{a.logn}, L = {L}, K = {K}, dnum = {DNUM}, plain modulus {PLAIN_MODULUS}; repairing chain; {a.num_symbols} symbols x {a.bits_per_symbol} bits per trial")
    missed = wrong = 0
    totals = {"corrected": 0, "uncorrectable": 0, "missed": 0, "exact": 0}
    for trial in range(a.trials):
        d_a = eng.upload(ct_a)
        n_sym = 0 if trial == 0 else a.num_symbols
        for idx in rng.integers(0, ct_a.size, n_sym):
            for bit in rng.choice(64, a.bits_per_symbol, replace=False):
                check(lib.fhe_flip_bit(eng._h, d_a.ptr, int(idx), int(bit), None))
        flipped = int(np.count_nonzero(d_a.download().reshape(-1) != ct_a.reshape(-1)))
        out, raised, tally = chain_repair(d_a)
        corrected = tally.get(F.SEAL_REPAIRED, 0)
        refused = tally.get(F.SEAL_UNCORRECTABLE, 0) + tally.get(F.SEAL_SUSPECT, 0)
        exact = bool((out == clean).all())
        miss = flipped > 0 and corrected == 0 and raised == 0
        missed += miss
        wrong += flipped > 0 and raised == 0 and not exact      # said to be all corrected, yet the result differs
        assert flipped > 0 or (exact and corrected == 0 and raised == 0), "the control trial differs from the clean run"
        verdict = "missed" if miss else "uncorrectable" if raised else "corrected" if corrected else "clean"
        for k, v in (("corrected", verdict == "corrected"), ("uncorrectable", verdict == "uncorrectable"), ("missed", miss), ("exact", exact)):
            totals[k] += int(v)
        print(f"trial {trial:3d}: flipped words {flipped:3d}, rows corrected {corrected:3d}, rows uncorrectable or suspect {refused:3d}, raised flag words {raised:4d}, "
              f"{verdict}, final words equal the fault-free run: {'yes' if exact else 'no'}", flush=True)
    eng.check()
    print(f"summary: {a.trials} trials (one control): {totals['corrected']} corrected, {totals['uncorrectable']} uncorrectable, {totals['missed']} missed; "
          f"{totals['exact']} final results equal the fault-free run bit for bit; {wrong} reported corrected with a differing result")
    return 1 if missed or wrong else 0


def main_fused_key(a, eng):
    """the reference's fault model on the relinearisation key at rest, through hmult_sealed_fused_key"""
    N, M = 1 << a.logn, L + K
    qs = F.create_moduli(N, [50] * M)
    rng = np.random.default_rng(a.seed)
    t = eng.tables(a.logn, qs)
    ks, ab = F.KeySwitch(eng, t, L, K, DNUM), F.Abft(eng, t)
    ks.set_plain_modulus(PLAIN_MODULUS)
    assert ks.apply_sealed_layout()["fused"]
    poly = lambda moduli: np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in moduli])
    ops = [eng.upload(poly(qs[:L])) for _ in range(4)]
    rlk = np.stack([np.stack([poly(qs) for _ in range(2)]) for _ in range(DNUM)])
    seals = [t.seal(d, limbs=L) for d in ops]
    s_rlk = ks.seal_key(eng.upload(rlk))

    def run(call, d_rlk):
        o0, o1, so, fl = call(*ops, d_rlk, ab, seals=seals, key_seal=s_rlk)
        return np.concatenate([o0.download().reshape(-1), o1.download().reshape(-1)]), fl

    clean, fl = run(ks.hmult_sealed_fused_key, eng.upload(rlk))
    ref, rfl = run(ks.hmult_sealed, eng.upload(rlk))
    assert nonzero(fl) == 0 and nonzero(rfl) == 0 and (clean == ref).all(), "the clean fused multiply differs from the sealed multiply"
    print(f"N = 2^{a.logn}, L = {L}, K = {K}, dnum = {DNUM}, plain modulus {PLAIN_MODULUS}; multiply: hmult_sealed_fused_key, flips in the relinearisation key "
          f"at rest; {a.num_symbols} symbols x {a.bits_per_symbol} bits per trial")
    missed = 0
    for trial in range(a.trials):
        d_rlk = eng.upload(rlk)
        n_sym = 0 if trial == 0 else a.num_symbols
        hit = set()
        for idx in rng.integers(0, rlk.size, n_sym):
            hit.add(int(idx) // N)
            for bit in rng.choice(64, a.bits_per_symbol, replace=False):
                check(lib.fhe_flip_bit(eng._h, d_rlk.ptr, int(idx), int(bit), None))
        flipped = int(np.count_nonzero(d_rlk.download().reshape(-1) != rlk.reshape(-1)))
        out, fl = run(ks.hmult_sealed_fused_key, d_rlk)
        corrupted = int(np.count_nonzero(out != clean))
        rows = np.flatnonzero(np.asarray(fl["key"]).reshape(-1)).tolist()
        raised = nonzero(fl)
        detected = raised > 0
        missed += flipped > 0 and not detected
        assert flipped > 0 or (corrupted == 0 and not detected), "the control trial differs from the clean run"
        assert rows == sorted(hit) or flipped == 0, "the raised key rows are not the rows that were flipped"
        print(f"trial {trial:3d}: flipped words {flipped:3d}, corrupted output words {corrupted:7d} of {out.size}, raised flag words {raised:4d}, key rows raised "
              f"{rows}, detected {'yes' if detected else 'no'}", flush=True)
    eng.check()
    print(f"summary: {a.trials} trials, {missed} with a flip and no flag")
    return 1 if missed else 0


def main_ntt(a, eng):
    """the trials of --ntt: the reference's flips in the forward transform's input at rest, through ntt_sealed"""
    N, B = 1 << a.logn, a.batch
    qs = F.create_moduli(N, [50] * B)
    rng = np.random.default_rng(a.seed)
    t = eng.tables(a.logn, qs)
    ab = F.Abft(eng, t)
    x = np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs])
    d_x = eng.upload(x)
    seal = t.seal(d_x, limbs=B)
    ref = eng.upload(x)
    t.forward(ref, limbs=B)
    clean = ref.download().reshape(B, N)
    poison = np.uint64((1 << 64) - 1)
    print(f"N = 2^{a.logn}, batch {B} (50-bit primes): ntt_sealed, flips in the transform's input at rest; {a.num_symbols} symbols x {a.bits_per_symbol} bits per trial")
    wrong = 0
    for trial in range(a.trials):
        d = eng.upload(x)
        n_sym = 0 if trial == 0 else a.num_symbols
        hit = set()
        for idx in rng.choice(x.size, n_sym, replace=False):
            hit.add(int(idx) // N)
            for bit in rng.choice(64, a.bits_per_symbol, replace=False):
                check(lib.fhe_flip_bit(eng._h, d.ptr, int(idx), int(bit), None))
        dst, seal_dst, fl = t.ntt_sealed(d, seal, ab, limbs=B)
        out = dst.download().reshape(B, N)
        corrupted = int(np.count_nonzero(out != clean))
        rows = np.flatnonzero(fl[0]).tolist()
        s_dst, s_ref = seal_dst.download().reshape(B, 2), t.seal(dst, limbs=B).download().reshape(B, 2)
        poisoned = [r for r in range(B) if (s_dst[r] == poison).all()]
        sealed = all((s_dst[r] == s_ref[r]).all() for r in range(B) if r not in poisoned)
        refused = np.flatnonzero(t.seal_verify(dst, seal_dst, limbs=B)).tolist()
        ok = rows == sorted(hit) and not fl[1].any() and poisoned == rows and refused == rows and sealed
        wrong += not ok
        assert n_sym > 0 or (ok and corrupted == 0), "the control trial raised a flag, or its seals are not seal(dst)"
        print(f"trial {trial:3d}: flipped rows {sorted(hit)}, corrupted output words {corrupted:7d} of {out.size} (symbol error rate {corrupted / out.size:.3f}), "
              f"input rows raised {rows}, ABFT words raised {int(np.count_nonzero(fl[1]))}, output seals poisoned {poisoned}, refused by seal_verify {refused}: "
              f"{'ok' if ok else 'WRONG'}", flush=True)
    eng.check()
    print(f"summary: {a.trials} trials (one control), {wrong} whose raised rows, poisoned seals or refused rows are not exactly the flipped rows")
    return 1 if wrong else 0


def main_polymul(a, eng):
    """the trials of --polymul: the reference's flips in a factor of the product at rest, through polymul_sealed"""
    N, B = 1 << a.logn, a.batch
    qs = F.create_moduli(N, [50] * B)
    rng = np.random.default_rng(a.seed)
    t = eng.tables(a.logn, qs)
    ab = F.Abft(eng, t)
    xa, xb = (np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs]) for _ in range(2))
    seal_a, seal_b = t.seal(eng.upload(xa), limbs=B), t.seal(eng.upload(xb), limbs=B)
    ref = eng.alloc(B * N)
    t.polymul(ref, eng.upload(xa), eng.upload(xb), limbs=B)
    clean = ref.download().reshape(B, N)
    poison = np.uint64((1 << 64) - 1)
    print(f"N = 2^{a.logn}, batch {B} (50-bit primes): polymul_sealed, flips in a factor at rest; {a.num_symbols} symbols x {a.bits_per_symbol} bits per trial")
    wrong = 0
    for trial in range(a.trials):
        d = [eng.upload(xa), eng.upload(xb)]
        n_sym = 0 if trial == 0 else a.num_symbols
        hit = [set(), set()]
        for idx in rng.choice(2 * xa.size, n_sym, replace=False):
            op, at = int(idx) // xa.size, int(idx) % xa.size
            hit[op].add(at // N)
            for bit in rng.choice(64, a.bits_per_symbol, replace=False):
                check(lib.fhe_flip_bit(eng._h, d[op].ptr, at, int(bit), None))
        c = eng.alloc(B * N)
        seal_c, fl = ab.polymul_sealed(c, d[0], d[1], seal_a, seal_b, limbs=B)
        out = c.download().reshape(B, N)
        corrupted = int(np.count_nonzero(out != clean))
        rows = [np.flatnonzero(fl["a"]).tolist(), np.flatnonzero(fl["b"]).tolist()]
        s_c, s_ref = seal_c.download().reshape(B, 2), t.seal(c, limbs=B).download().reshape(B, 2)
        poisoned = [r for r in range(B) if (s_c[r] == poison).all()]
        sealed = all((s_c[r] == s_ref[r]).all() for r in range(B) if r not in poisoned)
        refused = np.flatnonzero(t.seal_verify(c, seal_c, limbs=B)).tolist()
        both = sorted(hit[0] | hit[1])
        ok = rows == [sorted(hit[0]), sorted(hit[1])] and not fl["checked"].any() and poisoned == both and refused == both and sealed
        wrong += not ok
        assert n_sym > 0 or (ok and corrupted == 0), "the control trial raised a flag, or its seals are not seal(c)"
        print(f"trial {trial:3d}: flipped rows a {sorted(hit[0])} b {sorted(hit[1])}, corrupted product words {corrupted:7d} of {out.size} (symbol error rate "
              f"{corrupted / out.size:.3f}), rows raised a {rows[0]} b {rows[1]}, ABFT words raised {int(np.count_nonzero(fl['checked']))}, output seals poisoned "
              f"{poisoned}, refused by seal_verify {refused}: {'ok' if ok else 'WRONG'}", flush=True)
    eng.check()
    print(f"summary: {a.trials} trials (one control), {wrong} whose raised rows, poisoned seals or refused rows are not exactly the flipped rows")
    return 1 if wrong else 0


def main_bsgs(a, eng):
    """the trials of --bsgs: the reference's flips in a diagonal or a giant key at rest, through bsgs_matvec_sealed"""
    N, n1, n2 = 1 << a.logn, 4, 4
    qs = F.create_moduli(N, [50] * (L + K))
    rng = np.random.default_rng(a.seed)
    t = eng.tables(a.logn, qs)
    ks, ab = F.KeySwitch(eng, t, L, K, DNUM), F.Abft(eng, t)
    poly = lambda moduli: np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in moduli])
    key = lambda: np.stack([np.stack([poly(qs) for _ in range(2)]) for _ in range(DNUM)])
    c0, c1 = eng.upload(poly(qs[:L])), eng.upload(poly(qs[:L]))
    diags = np.stack([np.stack([poly(qs[:L]) for _ in range(n1)]) for _ in range(n2)])
    baby_elts, giant_elts = [pow(5, b, 2 * N) for b in range(1, n1)], [pow(5, g * n1, 2 * N) for g in range(1, n2)]
    prepared = [ks.prepare_galois_key(eng.upload(key()), e) for e in baby_elts]
    giant = [key() for _ in giant_elts]
    d_diags, d_giant = eng.upload(diags), [eng.upload(k) for k in giant]
    # seals, taken once of the clean data: what travels with the ciphertext, the keys and the diagonals
    seals = (t.seal(c0, limbs=L), t.seal(c1, limbs=L))
    s_baby, s_giant, s_diag = [ks.seal_key(k) for k in prepared], [ks.seal_key(k) for k in d_giant], ks.seal_diagonals(d_diags, n1, n2)

    def run(dd, dg):
        o0, o1, _, fl = ks.bsgs_matvec_sealed(c0, c1, dd, n1, n2, baby_elts, prepared, giant_elts, dg, ab, seals=seals, baby_key_seals=s_baby,
                                              giant_key_seals=s_giant, diag_seal=s_diag)
        return np.concatenate([o0.download().reshape(-1), o1.download().reshape(-1)]), {k: nonzero(v) for k, v in fl.items()}

    clean, groups = run(d_diags, d_giant)
    assert not any(groups.values()), "the clean call raised a flag"
    print(f"N = 2^{a.logn}, L = {L}, K = {K}, dnum = {DNUM}, n1 = {n1}, n2 = {n2}: bsgs_matvec_sealed; {a.num_symbols} symbols x {a.bits_per_symbol} bits per trial")
    missed, tally = 0, {"diagonal": [0, 0], "giant key": [0, 0]}
    for trial in range(a.trials):
        target = "diagonal" if trial % 2 else "giant key"
        which = int(rng.integers(0, len(giant)))
        src = diags if target == "diagonal" else giant[which]
        d = eng.upload(src)
        n_sym = 0 if trial == 0 else a.num_symbols
        for idx in rng.integers(0, src.size, n_sym):
            for bit in rng.choice(64, a.bits_per_symbol, replace=False):
                check(lib.fhe_flip_bit(eng._h, d.ptr, int(idx), int(bit), None))
        flipped = int(np.count_nonzero(d.download().reshape(-1) != src.reshape(-1)))
        out, groups = run(d if target == "diagonal" else d_diags, d_giant if target == "diagonal" else d_giant[:which] + [d] + d_giant[which + 1:])
        corrupted = int(np.count_nonzero(out != clean))
        own = groups["diags" if target == "diagonal" else "giant_keys"]
        detected = own > 0
        missed += flipped > 0 and not detected
        if flipped:
            tally[target][0] += 1
            tally[target][1] += int(detected)
        assert flipped > 0 or (corrupted == 0 and not any(groups.values())), "the control trial differs from the clean run"
        print(f"trial {trial:3d}: {target:9s} flipped words {flipped:3d}, corrupted output words {corrupted:7d} of {out.size}, raised flag words "
              f"{', '.join(f'{k} {v}' for k, v in groups.items() if v) or 'none'}, detected {'yes' if detected else 'no'}", flush=True)
    eng.check()
    print(f"summary: {a.trials} trials (one control): " + ", ".join(f"{k} {v[1]} of {v[0]} detected on its own rows" for k, v in tally.items())
          + f"; {missed} with a flip and no flag")
    return 1 if missed else 0


class _View:
    """words [off, off + n) of a device array, as the wrappers take operands (a pointer; nothing is owned)"""

    def __init__(self, eng, d, off, n):
        import ctypes as C
        self.eng, self.ptr, self.size, self.shape, self._keep = eng, C.c_void_p(d.ptr.value + 8 * off), n, (n,), d


def _view(eng, d, off, n):
    return _View(eng, d, off, n)


if __name__ == "__main__":
    sys.exit(main())
