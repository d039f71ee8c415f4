"""CPU-only: the lane functions of the aggregate verify over ragged groups by random linear combination
(bls-bn254_amd/csrc/aggregate_rlc.h) and its plan (aggregate_rlc_plan.h) compiled for the host with -DBN_CHECK into a
stand-alone program (tests/hostsim/aggregate_rlc_host.cpp): the weight derivation against hashlib, the 32-step GLV product
against the oracle's [a + b lambda mod r] P, the plan against a Python model, and -- on the oracle alone -- the identity the call
rests on.  A test tool; the product has no CPU path."""
import hashlib
import os
import random
import subprocess

import pytest

from tests import hostsim_build, synth
from tests.aggregate_rlc_support import cut, failed_ranges, keys_repeat, pair_groups, segments, weight, weight_of_digest
from tests.helpers import IDENT1, glv_lambda

R = synth.R
FP12_ONE = bytes(31) + b"\x01" + bytes(352)
DST = b"BLS_SIG_BN254G1_XMD:SHA-256_SVDW_RO_NUL_"


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("agr")
    # built where the test may write: nothing is left in the tree
    exe = hostsim_build.build("aggregate_rlc_host.cpp", os.path.join(str(d), "aggregate_rlc_host"), shared=False)

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
    rnd = random.Random(9)
    cmds, want = [], []
    for g in (0, 1, 255, 256, (1 << 32) + 5, (1 << 64) - 1):
        seed, sig = bytes(rnd.randrange(256) for _ in range(32)), bytes(rnd.randrange(256) for _ in range(64))
        dg = hashlib.sha256(seed + b"AGRLC" + g.to_bytes(8, "little") + sig).digest()
        a, b = int.from_bytes(dg[:4], "big"), int.from_bytes(dg[4:8], "big")
        assert weight(seed, g, sig) == (a, b) and (a or b)
        cmds.append(["weight", seed.hex(), g, sig.hex()]); want.append([a, b])
    # the function that maps a digest to a weight: big-endian halves, and a = b = 0 becomes (1, 0)
    for dg, w in ((bytes(8) + b"\xff" * 24, (1, 0)), (bytes(4) + b"\x00\x00\x00\x02" + bytes(24), (0, 2)), (b"\x80" + bytes(31), (1 << 31, 0)),
                  (b"\xff" * 32, ((1 << 32) - 1, (1 << 32) - 1)), (bytes(range(1, 33)), (0x01020304, 0x05060708)), (bytes(3) + b"\x07" + bytes(28), (7, 0))):
        assert weight_of_digest(dg) == w
        cmds.append(["digest", dg.hex()]); want.append(list(w))
    assert [ints(r) for r in run(cmds)] == want


def test_the_32_step_glv_product_against_the_oracle(run, oracle):
    lam = glv_lambda()
    rnd = random.Random(5)
    gen = oracle.g1_generator()
    pts = [oracle.g1_mul(gen, rnd.randrange(1, R)) for _ in range(3)]
    top = (1 << 32) - 1
    weights = [(0, rnd.randrange(1, 1 << 32)), (rnd.randrange(1, 1 << 32), 0), (top, top), (1, 0), (0, 1), (1, 1), (1 << 31, 1 << 31), (0, 0)]
    weights += [(rnd.randrange(1 << 32), rnd.randrange(1 << 32)) for _ in range(4)]

    def mul(p, a, b):
        k = (a + b * lam) % R
        return oracle.g1_mul(p, k) if k else IDENT1

    cmds, want = [], []
    for i, (a, b) in enumerate(weights):
        for p in (pts[i % 3], gen):
            cmds.append(["mul", a, b, p.hex()]); want.append([mul(p, a, b).hex()])
    cmds.append(["mul", 12345, 678, IDENT1.hex()]); want.append([IDENT1.hex()])
    # the two interleaved chains compute what the single chain computes, each under its own weight
    for (a, b), (c, d) in zip(weights, weights[1:] + weights[:1]):
        cmds.append(["mul2", a, b, pts[0].hex(), c, d, pts[1].hex()]); want.append([mul(pts[0], a, b).hex(), mul(pts[1], c, d).hex()])
    assert run(cmds) == want


def test_signature_test(run, oracle):
    sig = oracle.g1_mul(oracle.g1_generator(), 12345)
    off = sig[:63] + bytes([sig[63] ^ 1])
    cases = ((sig, 1), (IDENT1, 0), (off, 0), (b"\xff" * 32 + sig[32:], 0), (sig[:32] + b"\xff" * 32, 0))
    assert run([["sigok", s.hex()] for s, _ in cases]) == [[str(w)] for _, w in cases]


def test_plan_against_the_model(run):
    cmds, want = [], []
    # the group of every pair: empty groups in front, in the middle and behind; offsets that do not start at 0
    for off in ([0, 0, 2, 3, 3, 6, 6], [5, 5, 7, 7, 8], [3, 4], [0, 0, 0]):
        cmds.append(["pairs", len(off) - 1] + off); want.append(pair_groups(off))
    # segment bounds: G not divisible by S, S == G, one segment
    for G, S in ((10, 4), (7, 3), (40, 4), (5, 5), (33, 32), (9, 1), (1, 1)):
        bound, seg_of = cut(G, S)
        assert bound[0] == 0 and bound[-1] == G and all(b > a for a, b in zip(bound, bound[1:])) and len(seg_of) == G
        assert max(b - a for a, b in zip(bound, bound[1:])) - min(b - a for a, b in zip(bound, bound[1:])) <= 1
        cmds.append(["cut", G, S]); want.append(bound + seg_of)
    # the S rule at N = 2u - 1, 2u and 4u (and beyond the cap), a fixed S, S > G, S = 1
    u = 8
    for setting, N, G, expect in ((0, 2 * u - 1, 100, 1), (0, 2 * u, 100, 1), (0, 4 * u, 100, 2), (0, 4 * u, 1, 1), (0, 1000 * u, 1000, 16),
                                  (0, 1000 * u, 10, 10), (4, 2 * u, 100, 4), (4, 2 * u, 3, 3), (4096, 50, 4097, 4096), (1, 1000 * u, 100, 1), (2, 5, 1, 1)):
        assert segments(setting, N, u, G) == expect
        cmds.append(["segments", setting, 16, N, u, G]); want.append([expect])
    for S_max, expect in ((64, 62), (256, 62), (8, 8)):
        cmds.append(["segments", 0, S_max, 1000, u, 100]); want.append([expect])
    # round 1 is taken when the keys repeat
    for N, uu, mx in ((16, 8, 65536), (15, 8, 65536), (1, 1, 65536), (2, 1, 65536), (200000, 65535, 65536), (200000, 65536, 65536)):
        cmds.append(["repeat", N, uu, mx]); want.append([int(keys_repeat(N, uu, mx))])
    # the ranges of the exact sub-calls: adjacent failed segments merged, trimmed to eligible groups, dropped when none is
    bound, _ = cut(12, 4)                                               # 0 3 6 9 12
    all_e = [1] * 12
    off3 = [5 + 3 * g for g in range(13)]
    for passed, elig in (([1, 1, 1, 1], all_e), ([0, 0, 0, 0], all_e), ([1, 0, 0, 1], all_e), ([0, 1, 0, 1], all_e), ([0, 1, 1, 0], all_e),
                         ([0, 1, 1, 1], [0, 0, 1] + [1] * 9), ([1, 1, 1, 0], [1] * 9 + [1, 0, 0]), ([1, 0, 1, 1], [1, 1, 1, 0, 0, 0] + [1] * 6),
                         ([0, 0, 1, 1], [0, 1, 0, 0, 1, 0] + [1] * 6), ([0], all_e)):
        bd = bound if len(passed) == 4 else [0, 12]
        for gap in (0, 12, 13, 1 << 16):                                # 3 pairs per group: 9 pairs + 3 signatures lie between segments 0 and 2
            n, ranges = failed_ranges(bd, passed, elig, off3, gap)
            cmds.append(["ranges", len(passed)] + bd + passed + [12] + elig + off3 + [gap]); want.append([n, len(ranges)] + [x for r in ranges for x in r])
    assert failed_ranges(bound, [1, 0, 0, 1], all_e) == (6, [(3, 9)])
    assert failed_ranges(bound, [0, 0, 1, 1], [0, 1, 0, 0, 1, 0] + [1] * 6) == (2, [(1, 5)])
    assert failed_ranges(bound, [1, 0, 1, 1], [1, 1, 1, 0, 0, 0] + [1] * 6) == (0, [])
    assert failed_ranges(bound, [0, 1, 0, 1], all_e, off3, 12) == (6, [(0, 3), (6, 9)])      # 9 pairs + 3 signatures between them
    assert failed_ranges(bound, [0, 1, 0, 1], all_e, off3, 13) == (9, [(0, 9)])
    assert [ints(r) for r in run(cmds)] == want


def test_the_identity_on_the_oracle_alone(oracle):
    """3 groups of (2, 1, 3) pairs over 2 keys: e(sum r_g sig_g, -G2gen) prod_k e(sum_{pk_gi = pk_k} r_g H_gi, pk_k) finishes to one
    exactly when all three groups are valid; with sig_0 + D and sig_1 - D (errors that cancel without weights) it does not"""
    lam = glv_lambda()
    sks = [synth.sk_of(0), synth.sk_of(1)]
    pks = [oracle.sk_to_pk(s) for s in sks]
    keys = [[0, 1], [0], [1, 0, 1]]
    msgs = [[synth.msg_of(10 * g + j) for j in range(len(ks))] for g, ks in enumerate(keys)]
    sigs = [oracle.aggregate_sigs(b"".join(oracle.sign(sks[k], m, DST) for k, m in zip(ks, ms)), len(ks)) for ks, ms in zip(keys, msgs)]
    neg_g2 = oracle.g2_mul(oracle.g2_generator(), R - 1)
    seed = bytes(range(32))

    def finishes_to_one(sigs):
        r = [(a + b * lam) % R for a, b in (weight(seed, g, s) for g, s in enumerate(sigs))]
        acc = {"sig": IDENT1, 0: IDENT1, 1: IDENT1}
        for g, (ks, ms) in enumerate(zip(keys, msgs)):
            acc["sig"] = oracle.g1_add(acc["sig"], oracle.g1_mul(sigs[g], r[g]))
            H = oracle.hash_to_g1_batch(ms, DST)
            for j, k in enumerate(ks):
                acc[k] = oracle.g1_add(acc[k], oracle.g1_mul(H[64 * j:64 * j + 64], r[g]))
        ml = oracle.multi_miller_loop(acc["sig"] + acc[0] + acc[1], neg_g2 + pks[0] + pks[1], 3)
        return oracle.final_exponentiation(ml, 1) == FP12_ONE

    for g in range(3):                                                  # the groups are valid one by one
        assert oracle.aggregate_verify(b"".join(pks[k] for k in keys[g]), msgs[g], sigs[g], DST)
    assert finishes_to_one(sigs)
    D = oracle.g1_mul(oracle.g1_generator(), 777)
    bad = [oracle.g1_add(sigs[0], D), oracle.g1_add(sigs[1], oracle.g1_mul(D, R - 1)), sigs[2]]
    assert oracle.aggregate_sigs(b"".join(bad), 3) == oracle.aggregate_sigs(b"".join(sigs), 3)       # unweighted, the errors cancel
    assert not finishes_to_one(bad)
    assert not finishes_to_one([sigs[0], sigs[2], sigs[1]])
