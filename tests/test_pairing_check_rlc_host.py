"""CPU-only: the lane functions of the pairing-product checks over ragged groups by random linear combination
(bls-bn254_amd/csrc/pairing_check_rlc.h) and its plan (pairing_check_rlc_plan.h over aggregate_rlc_plan.h) compiled for the host with
-DBN_CHECK into a stand-alone program (tests/hostsim/pairing_check_rlc_host.cpp): the weight derivation against hashlib, the
32-step product over affine entries against the oracle's [a + b lambda mod r] P, the pair and eligibility predicates against the
oracle's checks, the plan against a Python model, and -- on the oracle alone -- the identity the call rests on.  A test tool; the
product has no CPU path."""
import hashlib
import os
import random
import subprocess

import pytest

from tests import hostsim_build, point_cases, synth
from tests.helpers import IDENT1, IDENT2, b32, glv_lambda
from tests.pairing_check_rlc_support import (MAX_KEYS, MAX_SEGMENTS, MERGE_GAP, S_MAX, cut, failed_ranges, pair_truth, plan, round1, segments, weight,
                                             weight_of_digest)

R, P = synth.R, synth.P
FP12_ONE = bytes(31) + b"\x01" + bytes(352)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("pcr")
    # built where the test may write: nothing is left in the tree
    exe = hostsim_build.build("pairing_check_rlc_host.cpp", os.path.join(str(d), "pairing_check_rlc_host"), shared=False)

    def f(commands):
        """commands: lists of tokens -> per command the result line's tokens (without the command's name)"""
        path = os.path.join(str(d), "commands.txt")
        with open(path, "w") as fh:
            fh.write("\n".join(" ".join(str(t) for t in c) for c in commands) + "\n")
        out = subprocess.run([exe, path], check=True, stdout=subprocess.PIPE).stdout.decode().splitlines()
        assert len(out) == len(commands) and all(o.split()[0] == c[0] for o, c in zip(out, commands))
        return [o.split()[1:] for o in out]
    return f


def ints(tok):
    return [int(t) for t in tok]


def test_weights_against_hashlib(run):
    rnd = random.Random(19)
    cmds, want = [], []
    for g in (0, 1, 255, 256, (1 << 32) + 5, (1 << 64) - 1):
        seed = bytes(rnd.randrange(256) for _ in range(32))
        dg = hashlib.sha256(seed + b"PCRLC" + g.to_bytes(8, "little")).digest()
        a, b = int.from_bytes(dg[:4], "big"), int.from_bytes(dg[4:8], "big")
        assert weight(seed, g) == (a, b) and (a or b)
        cmds.append(["weight", seed.hex(), g]); want.append([a, b])
    # the function that maps a digest to a weight (aggregate_rlc.h's, reused): big-endian halves, and a = b = 0 becomes (1, 0)
    for dg, w in ((bytes(8) + b"\xff" * 24, (1, 0)), (bytes(4) + b"\x00\x00\x00\x02" + bytes(24), (0, 2)), (b"\x80" + bytes(31), (1 << 31, 0)),
                  (b"\xff" * 32, ((1 << 32) - 1, (1 << 32) - 1)), (bytes(range(1, 33)), (0x01020304, 0x05060708))):
        assert weight_of_digest(dg) == w
        cmds.append(["digest", dg.hex()]); want.append(list(w))
    assert [ints(r) for r in run(cmds)] == want


def test_the_weigh_chain_on_affine_inputs_against_the_oracle(run, oracle):
    lam = glv_lambda()
    rnd = random.Random(15)
    gen = oracle.g1_generator()
    pts = [oracle.g1_mul(gen, rnd.randrange(1, R)) for _ in range(3)]
    top = (1 << 32) - 1
    weights = [(0, rnd.randrange(1, 1 << 32)), (rnd.randrange(1, 1 << 32), 0), (top, top), (1, 0), (0, 1), (1, 1), (1 << 31, 1 << 31), (0, 0), (top, 0), (0, top),
               (top, 1), (1, top)]
    weights += [(rnd.randrange(1 << 32), rnd.randrange(1 << 32)) for _ in range(4)]

    def mul(p, a, b):
        k = (a + b * lam) % R
        return oracle.g1_mul(p, k) if k else IDENT1

    g2 = oracle.g2_generator()
    cmds, want = [], []
    for i, (a, b) in enumerate(weights):
        for p in (pts[i % 3], gen):
            cmds.append(["mul", a, b, p.hex()]); want.append([mul(p, a, b).hex()])
    # the two interleaved chains compute what the single chain computes, each under its own weight
    for (a, b), (c, d) in zip(weights, weights[1:] + weights[:1]):
        cmds.append(["mul2", a, b, pts[0].hex(), c, d, pts[1].hex()]); want.append([mul(pts[0], a, b).hex(), mul(pts[1], c, d).hex()])
    # the whole lane: a pair that counts, a skipped pair (identity P; identity Q), a pair of an ineligible equation
    a, b = weights[-1]
    for p, q, elig, w in ((pts[2], g2, 1, mul(pts[2], a, b)), (gen, g2, 1, mul(gen, a, b)), (IDENT1, g2, 1, IDENT1), (bytes(32) + b32(5), g2, 1, IDENT1),
                          (pts[2], IDENT2, 1, IDENT1), (pts[2], g2, 0, IDENT1)):
        cmds.append(["lane", p.hex(), q.hex(), a, b, elig]); want.append([w.hex()])
    assert run(cmds) == want


def test_pair_and_eligibility_predicates_against_the_oracle(run, oracle, pyref):
    named = point_cases.named_pairs(oracle, pyref)
    assert {(point_cases.g1_cases(oracle, pyref)[a][0], point_cases.g2_cases(oracle, pyref)[b][0]) for (a, b), _, _ in named} == \
        {(x, y) for x in point_cases.G1_CLASSES for y in point_cases.G2_CLASSES}
    rows = [(p, q) for _, p, q in named]
    # coordinates that do not decode (>= p), in every position; an identity by x = 0 keeps its y unread
    g1, g2 = oracle.g1_generator(), oracle.g2_generator()
    rows += [(b32(P) + g1[32:], g2), (g1[:32] + b32(P + 1), g2), (b"\xff" * 32 + g1[32:], IDENT2), (bytes(32) + b"\xff" * 32, g2)]
    rows += [(g1, g2[:k] + b"\xff" * 32 + g2[k + 32:]) for k in (0, 32, 64, 96)]
    rows += [(g1, bytes(64) + b"\xff" * 64), (g1, bytes(32) + b32(P) + g2[64:])]
    truth = [pair_truth(oracle, p, q) for p, q in rows]
    assert any(ok and not sk for ok, sk in truth) and any(ok and sk for ok, sk in truth) and any(not ok for ok, _ in truth)
    got = run([["pair", p.hex(), q.hex()] for p, q in rows])
    for (p, q), t, gt in zip(rows, truth, got):
        assert bool(int(gt[0])) == t[0], (p.hex(), q.hex())
        if t[0]:
            assert bool(int(gt[1])) == t[1], (p.hex(), q.hex())
    # an equation is eligible when all its pairs are OK: flag bytes OK = 1, SKIP = 2
    cases = (([], 1), ([1], 1), ([3], 1), ([1, 3, 1], 1), ([0], 0), ([2], 0), ([1, 1, 2, 1], 0), ([1] * 70 + [0], 0), ([3] * 70, 1))
    assert [ints(r) for r in run([["eligible", len(f)] + f for f, _ in cases])] == [[w] for _, w in cases]


def test_round1_rule_and_exact_ranges_against_the_model(run):
    cmds, want = [], []
    assert ints(run([["consts"]])[0]) == [S_MAX, MERGE_GAP, MAX_SEGMENTS]
    for N, u, mx in ((16, 8, MAX_KEYS), (15, 8, MAX_KEYS), (0, 0, MAX_KEYS), (1, 1, MAX_KEYS), (2, 1, MAX_KEYS), (200000, MAX_KEYS, MAX_KEYS), (200000, MAX_KEYS + 1, MAX_KEYS)):
        cmds.append(["round1", N, u, mx]); want.append([int(round1(N, u, mx))])
    assert round1(2, 1) and not round1(0, 0) and not round1(3, 2) and round1(1 << 17, MAX_KEYS) and not round1(1 << 20, MAX_KEYS + 1)
    u = 3
    for setting, N, G, expect in ((0, 2 * u, 100, 1), (0, 4 * u, 100, 2), (0, 1000 * u, 1000, S_MAX), (0, 100 * u, 1000, 50), (0, 1000 * u, 10, 10), (4, 2 * u, 100, 4), (4, 2 * u, 3, 3),
                                  (4096, 50, 4097, 4096), (1, 1000 * u, 100, 1)):
        assert segments(setting, N, u, G, S_MAX) == expect
        cmds.append(["segments", setting, S_MAX, N, u, G]); want.append([expect])
    for G, S in ((10, 4), (7, 3), (5, 5), (9, 1)):
        bound, seg_of = cut(G, S)
        cmds.append(["cut", G, S]); want.append(bound + seg_of)
    # the ranges given to the exact call: 12 equations of 2 pairs, offsets that do not start at 0, four segments
    G = 12
    off = [7 + 2 * g for g in range(G + 1)]
    all_e = [1] * G
    bound, _ = cut(G, 4)
    for passed, elig in (([1, 0, 1, 1], all_e), ([0, 1, 0, 1], all_e), ([0, 0, 0, 0], all_e), ([1, 0, 1, 1], [1, 1, 1, 0, 0, 0] + [1] * 6),
                         ([0, 1, 1, 0], [0, 1, 1] + [1] * 7 + [0, 0]), ([1, 1, 0, 0], [1] * 6 + [0, 1, 0, 0, 1, 0])):
        for gap in (0, 9, 10, MERGE_GAP):                               # 6 pairs + 3 equations lie between segments 0 and 2
            n, ranges = failed_ranges(bound, passed, elig, off, gap)
            cmds.append(["ranges", 4] + bound + passed + [G] + elig + off + [gap]); want.append([n, len(ranges)] + [x for r in ranges for x in r])
    assert failed_ranges(bound, [0, 1, 0, 1], all_e, off, 9) == (6, [(0, 3), (6, 9)])
    assert failed_ranges(bound, [0, 1, 0, 1], all_e, off, 10) == (9, [(0, 9)])
    # no second round: one range from the first to the last eligible equation
    n, ranges = failed_ranges([0, G], [0], [0, 1] + [1] * 9 + [0], off, MERGE_GAP)
    cmds.append(["ranges", 1, 0, G, 0, G] + [0, 1] + [1] * 9 + [0] + off + [MERGE_GAP]); want.append([10, 1, 1, 11])
    assert (n, ranges) == (10, [(1, 11)])
    assert [ints(r) for r in run(cmds)] == want
    # the call's model: round 1 passed: nothing more; failed with the default rule; failed with segments = 1
    assert plan(0, 24, 3, G, True, all_e, off) == (1, [], 0)
    assert plan(0, 24, 3, G, False, all_e, off, [1, 0, 1, 1]) == (4, [(3, 6)], 3)
    assert plan(1, 24, 3, G, False, all_e, off) == (1, [(0, 12)], 12)


def test_the_identity_on_the_oracle_alone(oracle):
    """two equations over the same Q with products e(T, Q) and e(-T, Q): each is false, their unweighted product is one, and the
    weighted combination prod_Q e(sum r_g P_gj, Q) is not; with T the identity both hold and it is"""
    lam = glv_lambda()
    G1, G2 = oracle.g1_generator(), oracle.g2_generator()
    Q, Q2 = oracle.g2_mul(G2, 31337), oracle.g2_mul(G2, 4242)
    A = oracle.g1_mul(G1, 1234567)
    negA_scaled = oracle.g1_mul(G1, (-1234567 * 4242 * pow(31337, -1, R)) % R)       # e(A, Q2) e(negA_scaled, Q) = 1
    T = oracle.g1_mul(G1, 777)
    negT = oracle.g1_mul(T, R - 1)
    seed = bytes(range(32))

    def one(ml):
        return oracle.final_exponentiation(ml, 1) == FP12_ONE

    def combined(eqs):
        r = [(a + b * lam) % R for a, b in (weight(seed, g) for g in range(len(eqs)))]
        acc = {Q: IDENT1, Q2: IDENT1}
        for g, eq in enumerate(eqs):
            for p, q in eq:
                acc[q] = oracle.g1_add(acc[q], oracle.g1_mul(p, r[g]))
        return one(oracle.multi_miller_loop(acc[Q] + acc[Q2], Q + Q2, 2))

    good = [[(A, Q2), (negA_scaled, Q)], [(negA_scaled, Q), (A, Q2)]]
    for eq in good:
        assert one(oracle.multi_miller_loop(b"".join(p for p, _ in eq), b"".join(q for _, q in eq), 2))
    assert combined(good)
    bad = [good[0] + [(T, Q)], good[1] + [(negT, Q)]]
    for eq in bad:
        assert not one(oracle.multi_miller_loop(b"".join(p for p, _ in eq), b"".join(q for _, q in eq), 3))
    both = bad[0] + bad[1]
    assert one(oracle.multi_miller_loop(b"".join(p for p, _ in both), b"".join(q for _, q in both), 6))      # unweighted, the errors cancel
    assert not combined(bad)
    assert not combined([bad[0], good[1]])
