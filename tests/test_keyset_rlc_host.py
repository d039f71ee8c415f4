"""CPU-only: the plan of the key-set FastAggregateVerify by random linear combination per message
(bls-bn254_amd/csrc/keyset_rlc_plan.h) and its lane functions (keyset_rlc.h) compiled for the host with -DBN_CHECK into a
stand-alone program (tests/hostsim/keyset_rlc_host.cpp): the plan against a Python model and against its own invariants, the
64-bit multiplication in G2 (and G1) against the pure-Python curve arithmetic, the weight derivation against hashlib, the
eligibility predicate on hand-made words, and the states of a chunk.  A test tool; the product has no CPU path."""
import hashlib
import os
import random
import subprocess

import pytest

from tests import hostsim_build
from tests.helpers import IDENT1, IDENT2
from tests.keyset_support import rlc_model_plan

RUN = 16                                                                # keyset_rlc_plan.h KSR_RUN


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("ksr")
    # built where the test may write: nothing is left in the tree
    exe = hostsim_build.build("keyset_rlc_host.cpp", os.path.join(str(d), "keyset_rlc_host"), shared=False)

    def f(commands):
        """commands: lists of tokens -> per command the result line's tokens (without the command's name)"""
        path = os.path.join(str(d), "commands.txt")
        with open(path, "w") as fh:
            fh.write("\n".join(" ".join(str(t) for t in c) for c in commands) + "\n")
        out = subprocess.run([exe, path], check=True, stdout=subprocess.PIPE).stdout.decode().splitlines()
        assert len(out) == len(commands) and all(o.split()[0] == c[0] for o, c in zip(out, commands))
        return [o.split()[1:] for o in out]
    return f


def hexs(b):
    return bytes(b).hex() or "-"


def model_levels(chunks):
    """plan_seg_levels over the chunks in runs of RUN: per level the (start, len) runs"""
    levels, seg = [], [(s, s + l) for s, l, _ in chunks]
    while True:
        runs, nxt = [], []
        for a, b in seg:
            first = len(runs)
            runs += [(s, min(RUN, b - s)) for s in range(a, b, RUN)]
            nxt.append((first, len(runs)))
        levels.append(runs)
        if len(runs) == len(seg):
            return levels
        seg = nxt


def parse_plan(tok, G):
    v = [int(t) for t in tok]
    n_cls, n_chunks, n_levels, n_multi, items_max = v[:5]
    at = 5
    order, pos, chunk_of, multi = (v[at + k * G:at + (k + 1) * G] for k in range(4))
    at += 4 * G
    rep = v[at:at + n_cls]; at += n_cls
    chunks = [tuple(v[at + 3 * i:at + 3 * i + 3]) for i in range(n_chunks)]; at += 3 * n_chunks
    levels = []
    for _ in range(n_levels):
        cnt = v[at]; at += 1
        levels.append([tuple(v[at + 2 * i:at + 2 * i + 2]) for i in range(cnt)]); at += 2 * cnt
    assert at == len(v)
    return dict(order=order, pos=pos, chunk_of=chunk_of, multi=multi, rep=rep, chunks=chunks, levels=levels, n_multi=n_multi, items_max=items_max)


@pytest.mark.parametrize("C", [2, 64])
def test_plan_against_the_model_and_its_invariants(run, C):
    rnd = random.Random(C)
    sizes = [1, C - 1, C, C + 1, 2 * C + 1]
    msgs = []
    for k, s in enumerate(sizes):
        msgs += [b"class %d" % k] * s
    # classes by BYTE equality: a last byte that differs, a message that is a prefix of another, the empty message twice
    msgs += [b"slot 7a", b"slot 7b", b"slot 7a", b"slot", b"slot 7", b"", b"", b"slot 7b"]
    rnd.shuffle(msgs)
    G = len(msgs)
    p = parse_plan(run([["plan", C, G] + [hexs(m) for m in msgs]])[0], G)
    order, chunks, rep = rlc_model_plan(msgs, C)
    assert p["order"] == order and p["chunks"] == chunks and p["rep"] == rep
    assert len(rep) == len(set(msgs)) == len(sizes) + 5
    # a stable permutation and its inverse
    cls = [rep.index(msgs.index(m)) for m in msgs]
    assert sorted(order) == list(range(G)) and all(p["pos"][order[i]] == i for i in range(G))
    assert all((cls[a], a) < (cls[b], b) for a, b in zip(order, order[1:]))
    assert all(msgs[rep[k]] == msgs[g] for g, k in enumerate(cls)) and rep == sorted(rep)
    # every group in exactly one chunk, no chunk over two classes or over C groups, chunks tile the sorted positions
    at = 0
    for ch, (s, l, k) in enumerate(chunks):
        assert s == at and 1 <= l <= C and {cls[order[i]] for i in range(s, s + l)} == {k}
        assert all(p["chunk_of"][order[i]] == ch and p["multi"][order[i]] == int(l >= 2) for i in range(s, s + l))
        at += l
    assert at == G and p["n_multi"] == sum(l for _, l, _ in chunks if l >= 2)
    for k in range(len(rep)):                                           # a class is cut into ceil(size / C) chunks, all full but the last
        mine = [l for _, l, kk in chunks if kk == k]
        size = cls.count(k)
        assert len(mine) == -(-size // C) and all(l == C for l in mine[:-1]) and sum(mine) == size
    # the run descriptors tile each chunk, level by level, down to one item per chunk
    levels = model_levels(chunks)
    assert p["levels"] == levels
    assert p["items_max"] == max([1] + [len(lv) for lv in levels[:-1]])
    seg = [(s, s + l) for s, l, _ in chunks]
    for runs in p["levels"]:
        it = iter(runs)
        nxt, n = [], 0
        for a, b in seg:
            first, x = n, a
            while x < b:
                s, l = next(it)
                assert s == x and 1 <= l <= RUN
                x += l; n += 1
            nxt.append((first, n))
        assert next(it, None) is None
        seg = nxt
    assert len(p["levels"][-1]) == len(chunks)
    assert (len(levels) == 1) == (C <= RUN)


def test_plan_of_distinct_messages_and_of_one_message(run):
    """classes of one: every chunk has one member and nothing is worth weighing; one class of 129 at C = 64: 64 + 64 + 1"""
    msgs = [b"m%d" % g for g in range(20)]
    res = run([["plan", 64, 20] + [hexs(m) for m in msgs], ["plan", 64, 129] + [hexs(b"same")] * 129])
    p = parse_plan(res[0], 20)
    assert p["n_multi"] == 0 and p["chunks"] == [(g, 1, g) for g in range(20)] and p["order"] == list(range(20)) and p["multi"] == [0] * 20
    p = parse_plan(res[1], 129)
    assert p["chunks"] == [(0, 64, 0), (64, 64, 0), (128, 1, 0)] and p["n_multi"] == 128 and p["multi"] == [1] * 128 + [0]


def test_the_64_bit_multiplication_against_the_curve_model(run, pyref):
    B = pyref
    rnd = random.Random(5)
    scalars = [1, 2, 1 << 63, (1 << 64) - 1] + [rnd.randrange(1, 1 << 64) for _ in range(4)]
    Q = B.g2_mul(B.G2_GEN, rnd.randrange(1, B.R))
    S = B.g1_mul(B.G1_GEN, rnd.randrange(1, B.R))
    cmds, want = [], []
    for r in scalars:
        cmds.append(["mulg2", r, hexs(B.g2_to_bytes(Q))]); want.append([B.g2_to_bytes(B.g2_mul(Q, r)).hex()])
        cmds.append(["mulg2", r, hexs(IDENT2)]); want.append([IDENT2.hex()])
        cmds.append(["mulg1", r, hexs(B.g1_to_bytes(S))]); want.append([B.g1_to_bytes(B.g1_mul(S, r)).hex()])
    cmds.append(["mulg1", scalars[-1], hexs(IDENT1)]); want.append([IDENT1.hex()])
    assert run(cmds) == want


def test_weights_against_hashlib(run):
    rnd = random.Random(9)
    cmds, want = [], []
    for g in (0, 1, 255, 256, (1 << 32) + 5, (1 << 64) - 1):
        seed, sig = bytes(rnd.randrange(256) for _ in range(32)), bytes(rnd.randrange(256) for _ in range(64))
        dg = hashlib.sha256(seed + b"KSRLC" + g.to_bytes(8, "little") + sig).digest()
        cmds.append(["weight", hexs(seed), g, hexs(sig)]); want.append([str(int.from_bytes(dg[:8], "big") or 1)])
    # the function that maps a digest to a weight: big-endian, and 0 becomes 1
    for dg, w in ((bytes(8) + b"\xff" * 24, 1), (bytes(7) + b"\x02" + bytes(24), 2), (b"\x80" + bytes(31), 1 << 63), (b"\xff" * 32, (1 << 64) - 1),
                  (bytes(range(1, 33)), 0x0102030405060708)):
        cmds.append(["digest", hexs(dg)]); want.append([str(w)])
    assert run(cmds) == want


def test_eligibility_on_hand_made_words(run, pyref):
    B = pyref
    n = 70                                                              # three words, the last of 6 keys

    def row(bits):
        r = bytearray((n + 7) // 8)
        for i in bits:
            r[i >> 3] |= 1 << (i & 7)
        return hexs(r)

    def words(bits):
        return [sum(1 << (i - 32 * w) for i in bits if i // 32 == w) for w in range(3)]

    everyone = set(range(n))
    skip, invalid = {3, 40}, {3, 9, 40, 69}                             # 3 and 40 are skipped (never added); 9 and 69 are added but lack KeyValidate
    valid = words(everyone - invalid)
    cases = [(set(), 1), ({0, 1, 68}, 1), ({3}, 1), ({3, 40, 5}, 1), ({9}, 0), ({0, 69}, 0), ({31, 32, 63, 64}, 1), (everyone - {9, 69}, 1), (everyone, 0)]
    cmds = [["rowvalid", n, row(r)] + words(skip) + valid for r, _ in cases]
    want = [[str(w)] for _, w in cases]
    # bits past the last key in the words change nothing
    cmds.append(["rowvalid", n, row({64})] + words(skip) + [valid[0], valid[1], valid[2] & 0x3f]); want.append(["1"])
    # the predicate: all four conditions
    for v in range(16):
        a = [(v >> k) & 1 for k in range(4)]
        cmds.append(["elig"] + a); want.append([str(int(a[0] and a[1] and a[2] and not a[3]))])
    # the signature: on the curve and not the identity
    sig = B.g1_to_bytes(B.g1_mul(B.G1_GEN, 12345))
    off = sig[:63] + bytes([sig[63] ^ 1])
    for s, w in ((sig, 1), (IDENT1, 0), (off, 0), (b"\xff" * 32 + sig[32:], 0), (sig[:32] + b"\xff" * 32, 0)):
        cmds.append(["sigok", hexs(s)]); want.append([str(w)])
    assert run(cmds) == want


def test_chunk_states(run, pyref):
    """state 2: the weighted G2 sum of a chunk is the identity (P and -P under the same weight); state 0: fewer than two eligible
    members; state 1 otherwise.  An ineligible member contributes the identity whatever it holds."""
    B = pyref
    Pt = B.g2_mul(B.G2_GEN, 777)
    Q = B.g2_mul(B.G2_GEN, 778)
    p, neg, q = (hexs(B.g2_to_bytes(x)) for x in (Pt, B.g2_neg(Pt), Q))
    cmds = [["chunk", 2, 1, 5, p, 1, 5, neg],                           # cancels: degenerate
            ["chunk", 2, 1, 5, p, 1, 6, neg],                           # different weights: does not
            ["chunk", 3, 1, 5, p, 0, 5, neg, 1, 9, q],                  # the ineligible member is not added
            ["chunk", 2, 1, 5, p, 0, 5, q],                             # one eligible member
            ["chunk", 2, 0, 5, p, 0, 5, q],
            ["chunk", 3, 1, 5, p, 1, 5, neg, 1, 1, q]]
    assert run(cmds) == [["2", "1", "2"], ["2", "0", "1"], ["2", "0", "1"], ["1", "0", "0"], ["0", "1", "0"], ["3", "0", "1"]]
