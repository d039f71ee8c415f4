"""GPU tests (MI355X) of the checked merge of partial aggregates per committee of a registered key set
(blsbn254_keyset_committee_merge_checked_batch).  The yardstick throughout is the EXISTING full-width call
Engine.keyset_merge_checked_batch on the contribution rows scattered over the registry, on the same handle: signatures, statuses
and used flags byte for byte, the committee rows against the full-width rows read through the member lists.  Beside it the
sequential model of tests/test_gpu_keyset_merge.py (used flags, statuses, counters), the oracle's aggregate of the used
signatures, and the committee verify on every status-0 group."""
import ctypes
import random

import numpy as np
import pytest

import blsbn254_loader
from tests import synth
from tests.gpu_support import eng, fresh_engine, M
from tests.helpers import bits_of, IDENT1, row_of
from tests.keyset_support import as_args, chunks, com_args, Committee, compact, Con, delta, expect, keys_of, sign_all, sign_positions, ST_SHORT, STATS, World

pytestmark = pytest.mark.gpu
E_ARG = -1
R = synth.R
_M = blsbn254_loader.load()
_M.Engine.keyset_committee_merge_checked_batch              # the feature is there, or this module does not import
ZERO = dict.fromkeys(STATS, 0)


@pytest.fixture(scope="module")
def W(eng, M):
    return World(eng, M)


@pytest.fixture(scope="module")
def handles(eng, M, W):
    hs = {False: W.keyset(M, eng, False), True: W.keyset(M, eng, True)}
    yield hs
    for ks in hs.values():
        ks.close()


def siblings(e):
    return e.keyset_stats(), e.keyset_aggregate_stats(), e.keyset_committee_stats(), e.keyset_committee_aggregate_stats(), e.keyset_merge_stats()


def yardstick(e, ks, n, coms, com, groups, msgs, dst):
    """the full-width call on the scattered rows (the wrapper scatters key indices), its rows read through the member lists"""
    out, wide, used, st = e.keyset_merge_checked_batch(ks, as_args(groups), msgs, dst)
    rbw = (n + 7) // 8
    return out, [compact(coms[c], wide[rbw * g:rbw * g + rbw]) for g, c in enumerate(com)], used, st


def check_model(oracle, coms, com, groups, res, kinds=None):
    """res against the sequential model; returns the stats the call must have added"""
    tally = dict.fromkeys(STATS, 0)
    assert len(res[0]) == 64 * len(groups) and len(res[1]) == len(groups) == len(res[2]) == len(res[3])
    for g, (c, cs) in enumerate(zip(com, groups)):
        used, union, fb, verified = expect(cs, kinds[g] if kinds else None)
        sig, rb = res[0][64 * g:64 * g + 64], (len(coms[c]) + 7) // 8
        tally["fallback_groups"] += fb; tally["verified_contributions"] += verified
        assert res[2][g] == used and len(res[1][g]) == rb, g
        if union is None:
            assert res[3][g] == ST_SHORT and sig == IDENT1 and res[1][g] == bytes(rb), g
            tally["short_groups"] += 1
            continue
        tally["optimistic_groups"] += not fb
        kept = [x.sig for x, u in zip(cs, used) if u]
        assert res[3][g] == 0 and res[1][g] == row_of({coms[c].index(k) for k in union}, len(coms[c])), g
        assert sig == oracle.aggregate_sigs(b"".join(kept), len(kept)), g
    return tally


def run_both(e, oracle, ks, W, com, groups, msgs, kinds=None):
    """the call, equal to the yardstick and the model; returns (result, stats delta of the call)"""
    sib0, s0 = siblings(e), e.keyset_committee_merge_stats()
    res = e.keyset_committee_merge_checked_batch(ks, com, com_args(W.coms, com, groups), msgs, W.dst)
    s1 = e.keyset_committee_merge_stats()
    assert siblings(e) == sib0                                            # the siblings' counters are left alone
    y0 = e.keyset_merge_stats()
    want = yardstick(e, ks, W.n, W.coms, com, groups, msgs, W.dst)
    y1 = e.keyset_merge_stats()
    assert res[3] == want[3] and res[0] == want[0] and res[2] == want[2] and res[1] == want[1]
    tally = check_model(oracle, W.coms, com, groups, res, kinds)
    assert delta(s1, s0) == delta(y1, y0) == tally
    bits = bits_of(e.keyset_committee_fast_aggregate_verify_batch(ks, com, res[1], msgs, res[0], W.dst), len(com))
    assert [bool(b) for b in bits] == [s == 0 for s in res[3]]             # the committee verify accepts exactly the status-0 groups
    return res, tally


def cut(keys, parts):
    """keys into `parts` contributions of nearly equal size, all of them"""
    k = max(1, len(keys) // parts)
    out = [keys[i:i + k] for i in range(0, k * (parts - 1), k)] + [keys[k * (parts - 1):]]
    return [x for x in out if x]


@pytest.mark.parametrize("checked", [False, True])
def test_all_honest_and_disjoint(eng, oracle, W, handles, checked):
    ks = handles[checked]
    rnd = random.Random(11)
    shaped = []
    for c in range(len(W.coms)):
        clean = keys_of(W, c)
        rnd.shuffle(clean)
        shaped += [(c, []), (c, [Con(clean[:1])]), (c, [Con(x) for x in cut(clean, 4)]), (c, [Con(x) for x in cut(clean[:len(clean) // 2], 2)])]
    rnd.shuffle(shaped)
    com, groups = [c for c, _ in shaped], [cs for _, cs in shaped]
    assert sum(1 for a, b in zip(com, com[1:]) if a != b) > len(com) // 2         # the caller's order interleaves the committees
    whole = [g for g, (c, cs) in enumerate(shaped) if c in (1, 3, 5) and len(cs) == 4]
    assert len(whole) == 3 and all(set().union(*(x.keys for x in groups[g])) == set(W.coms[com[g]]) for g in whole)     # cover their whole committee
    msgs = [b"committee merge honest %d" % g for g in range(len(com))]
    sign_all(eng, W.reg, groups, msgs, W.dst)
    res, tally = run_both(eng, oracle, ks, W, com, groups, msgs)
    empty = sum(1 for cs in groups if not cs)
    assert empty == 7 and tally == dict(zip(STATS, (len(com) - empty, 0, 0, empty)))
    assert all(all(u) for u in res[2]) and list(res[3]) == [0 if cs else ST_SHORT for cs in groups]
    for g in whole:
        n = len(W.coms[com[g]])
        assert res[1][g] == row_of(range(n), n)
    # rows as bytes give the same
    assert eng.keyset_committee_merge_checked_batch(ks, com, com_args(W.coms, com, groups, as_rows=True), msgs, W.dst) == res
    # against the oracle's verify, on a group of the committee listed descending
    g = next(g for g in whole if com[g] == 3)
    assert oracle.fast_aggregate_verify(W.reg.gather(W.coms[3]), 33, msgs[g], res[0][64 * g:64 * g + 64], W.dst)


@pytest.mark.parametrize("checked", [False, True])
def test_left_out_without_fallback(eng, oracle, W, handles, checked):
    ks = handles[checked]
    at = W.reg.at
    A, B, X = chunks(keys_of(W, 1), [4, 3, 2])
    A2, B2, X2, Y2, Z2 = chunks(keys_of(W, 2), [4, 3, 2, 2, 2])
    A4, B4, X4, Y4, Z4, V4, U4 = chunks(keys_of(W, 4), [4, 3, 2, 2, 2, 2, 2])
    groups = [
        [Con(A), Con(A[2:] + X), Con(A), Con([], cand=False, good=False), Con(B)],                          # overlapping, duplicate, empty row
        [Con(A2), Con(X2), Con(Y2), Con(Z2), Con(B2)],                                                      # signatures that are no candidates
        [Con(A4), Con(X4 + [at["ident"]], cand=False), Con(Y4 + [at["off"]], cand=False), Con(Z4 + [at["undec"]], cand=False),
         Con(V4 + [at["nonsub"]], cand=False), Con(U4 + [12], cand=not checked), Con(B4)],                  # members without the KeyValidate bit
    ]
    com = [1, 2, 4]
    msgs = [b"committee merge left out %d" % g for g in range(3)]
    sign_all(eng, W.reg, groups, msgs, W.dst)
    s = groups[1]
    s[1].broken(IDENT1)
    s[2].broken(s[2].sig[:63] + bytes([s[2].sig[63] ^ 1]))                                                  # off the curve
    s[3].broken(b"\xff" * 32 + s[3].sig[32:])                                                               # does not decode
    res, tally = run_both(eng, oracle, ks, W, com, groups, msgs)
    assert res[2] == [[True, False, False, False, True], [True, False, False, False, True], [True, False, False, False, False, not checked, True]]
    assert tally == dict(zip(STATS, (3, 0, 0, 0)))


def test_one_wrong_contribution(eng, oracle, W, handles):
    ks = handles[False]
    com = [5, 1, 3, 2, 1, 0]
    shapes = {}
    for c in (5, 3, 1):
        A, K, C2, D = chunks(keys_of(W, c), [5, 4, 3, 2])
        shapes[c] = (Con(A), Con(K, sk_delta=1, good=False), Con(K[-1:] + C2), Con(D))
    a, bad, late, d = shapes[5]
    first = [bad, late, a, d]
    a, bad, late, d = shapes[3]
    middle = [a, bad, late, d]
    a, bad, late, d = shapes[1]
    last = [a, d, bad]
    A2, B2 = chunks(keys_of(W, 2), [6, 5])
    groups = [first, [Con(keys_of(W, 1)[20:25])], middle, [Con(A2), Con(B2)], last, [Con([20])]]
    msgs = [b"committee merge one wrong %d" % g for g in range(len(groups))]
    sign_all(eng, W.reg, groups, msgs, W.dst)
    res, tally = run_both(eng, oracle, ks, W, com, groups, msgs)
    # only the three groups with a wrong contribution went to the fallback; the later one that overlapped only it is used
    assert res[2] == [[False, True, True, True], [True], [True, False, True, True], [True, True], [True, True, False], [True]]
    assert tally == dict(zip(STATS, (3, 3, 11, 0)))
    # a group's outcome depends on its own inputs only: the honest neighbours alone
    others = [1, 3, 5]
    s0 = eng.keyset_committee_merge_stats()
    alone = eng.keyset_committee_merge_checked_batch(ks, [com[g] for g in others], com_args(W.coms, [com[g] for g in others], [groups[g] for g in others]),
                                                     [msgs[g] for g in others], W.dst)
    assert delta(eng.keyset_committee_merge_stats(), s0) == dict(zip(STATS, (3, 0, 0, 0)))
    assert alone == (b"".join(res[0][64 * g:64 * g + 64] for g in others), [res[1][g] for g in others], [res[2][g] for g in others], bytes(3))


def test_cancelling_errors_and_short_groups(eng, oracle, W, handles):
    ks = handles[False]
    at = W.reg.at
    A, B, C = chunks(keys_of(W, 2), [3, 2, 4])
    A5, B5 = chunks(keys_of(W, 5), [3, 2])
    groups = [
        [Con(A), Con(B), Con(C)],                                                    # two errors that cancel in the sum: both used
        [Con([at["p"]]), Con([at["negp"]])],                                         # each verifies, the kept keys are P and -P
        [Con(A5, sk_delta=3, good=False), Con(B5, sk_delta=5, good=False)],          # every candidate fails
        [Con(C)],
    ]
    com = [2, 4, 5, 2]
    msgs = [b"committee merge cancelling %d" % g for g in range(4)]
    sign_all(eng, W.reg, groups, msgs, W.dst)
    G = oracle.g1_generator()
    d = random.Random(162).randrange(1, R)
    a, b = groups[0][0], groups[0][1]
    a.sig = oracle.g1_add(a.sig, oracle.g1_mul(G, d)); a.good = False
    b.sig = oracle.g1_add(b.sig, oracle.g1_mul(G, R - d)); b.good = False
    pair = com_args(W.coms, [2, 2], [[a], [b]])
    assert eng.keyset_committee_fast_aggregate_verify_batch(ks, [2, 2], [row_of(pair[0][0][0], 32), row_of(pair[1][0][0], 32)], [msgs[0]] * 2, a.sig + b.sig,
                                                            W.dst) == b"\x00"       # neither verifies on its own
    res, tally = run_both(eng, oracle, ks, W, com, groups, msgs, kinds=["cancel", "zero_sum", None, None])
    assert res[2] == [[True, True, True], [False, False], [False, False], [True]] and res[3] == bytes([0, ST_SHORT, ST_SHORT, 0])
    assert tally == dict(zip(STATS, (2, 2, 4, 2)))


def test_order_matters(eng, oracle, W, handles):
    """the four orderings of tests/test_gpu_keyset_merge.py, as positions in the committee listed in descending order"""
    ks = handles[False]
    A, B, C = chunks(keys_of(W, 3), [4, 3, 5])
    a, ab, bc, c = Con(A), Con(A[-1:] + B), Con(B[-1:] + C), Con(C)
    groups = [[a, ab, bc, c], [c, bc, ab, a], [ab, a, c, bc], [bc, ab, a, c]]
    msgs = [b"committee merge order"] * 4
    sign_all(eng, W.reg, [[a, ab, bc, c]], msgs, W.dst)
    res, tally = run_both(eng, oracle, ks, W, [3] * 4, groups, msgs)
    assert res[2] == [[True, False, True, False]] * 4 and tally["optimistic_groups"] == 4
    pos = lambda keys: row_of({W.pos_of(3, k) for k in keys}, 33)
    assert res[1] == [pos(A + B[-1:] + C), pos(C + A[-1:] + B), pos(A[-1:] + B + C), pos(B[-1:] + C + A)]
    assert res[1][0] != res[1][1] and res[1][2] == res[1][1] and res[1][3] == res[1][0]       # two outcomes, by the order alone


def boundary_case(eng, W, tag=b""):
    """six groups with 0 to 9 contributions over six committees; group 0 needs the fallback, which then uses a contribution it
    had left out"""
    A, K, C2, D, E, F, G, H, I = chunks(keys_of(W, 5), [7, 4, 3, 2, 6, 1, 2, 2, 2])
    A1, B1, E1 = chunks(keys_of(W, 1), [4, 3, 2])
    F4, E4, D4, K4 = chunks(keys_of(W, 4), [1, 3, 2, 5])
    A3, K3, C3, D3, E3, F3 = chunks(keys_of(W, 3), [9, 4, 3, 2, 6, 1])
    com = [5, 1, 2, 4, 0, 3]
    groups = [
        [Con(A), Con(K, sk_delta=1, good=False), Con(K[:1] + C2), Con(D), Con(A[:2]), Con(E + F), Con(G), Con(H), Con(I)],
        [Con(B1), Con(A1), Con(B1[:1] + E1)],
        [],
        [Con(F4), Con(E4 + [W.reg.at["off"]], cand=False), Con(D4), Con(K4)],
        [Con([20])],
        [Con(A3), Con(K3), Con(C3), Con(D3), Con(E3), Con(F3)],
    ]
    msgs = [b"committee merge launch boundaries %d" % g + tag for g in range(len(groups))]
    return com, sign_all(eng, W.reg, groups, msgs, W.dst), msgs


BOUNDARY_STATS = dict(zip(STATS, (4, 1, 9, 1)))


def test_launch_boundaries(eng, oracle, M, W, handles, monkeypatch):
    """contexts with 8 and 16 lanes per launch and the default: the cuts fall inside a group's contributions (23 of them) and
    between groups (a group per select launch); under 8 lanes the fallback's per-contribution pass (nine candidates) is cut too"""
    com, groups, msgs = boundary_case(eng, W)
    want, tally = run_both(eng, oracle, handles[False], W, com, groups, msgs)
    assert tally == BOUNDARY_STATS and want[2][0] == [True, False, True, True, False, True, True, True, True]
    for chunk in (None, "8", "16"):
        e = fresh_engine(M, monkeypatch, chunk)
        try:
            ks = W.keyset(M, e, False)
            assert e.keyset_committee_merge_stats() == ZERO
            assert e.keyset_committee_merge_checked_batch(ks, com, com_args(W.coms, com, groups), msgs, W.dst) == want, chunk
            assert e.keyset_committee_merge_stats() == BOUNDARY_STATS
            if chunk == "8":
                nine = [0] * 9
                with pytest.raises(M.Bn254Error):
                    e.keyset_committee_merge_checked_batch(ks, nine, [[]] * 9, [b"m"] * 9, W.dst)
                assert b"launch chunk" in e._lib.blsbn254_last_error(e._ctx)
            ks.close()
        finally:
            e.close()


def test_more_than_64_words(eng, oracle, M):
    """a registry of 2100 keys and one committee that lists all of them in REVERSE order: rows of 66 words (263 bytes), the union
    kept in the merged row; the positions at which lanes change hands (lane 63's word, lane 0's second word) are those of the
    full-width test, reached through the reversed list.  A second committee of 40 members keeps its union in a register in the
    same call.  Validity by the committee verify; bytes by the yardstick, the oracle's aggregate and the model"""
    dst = M.DEFAULT_DST
    n = 2100
    reg = Committee(eng, n, 231)
    at = reg.at
    coms = [list(range(n - 1, -1, -1)), list(range(100, 180, 2))]
    key = lambda p: n - 1 - p                                           # position -> key of committee 0
    ok = lambda p: key(p) not in reg.unsignable and key(p) not in (at["ident"], at["negp"])
    lo, mid, hi = [p for p in range(700) if ok(p)], [p for p in range(700, 2040) if ok(p)], [p for p in range(2052, 2099) if ok(p)]
    edge = [2040, 2047, 2048, 2051]                                      # lane 63's word and lane 0's second word
    assert all(ok(p) for p in edge + [2099, 0]) and not ok(1) and key(1) == at["undec"]
    K = lambda ps: [key(p) for p in ps]
    forty = coms[1]
    groups = [
        [Con(K(lo)), Con(K(mid)), Con(K(edge)), Con(K(hi)), Con(K([2047, hi[3]])), Con(K([2099]))],
        [Con(forty[:7]), Con(forty[5:9]), Con(forty[9:])],
        [Con(K(mid)), Con(K(lo), sk_delta=1, good=False), Con(K([3 * k for k in range(10, 200) if ok(3 * k)])), Con(K(edge[:2] + [1]), cand=False), Con(K(edge[2:])),
         Con(K([2048]))],
        [Con(K([2099])), Con(K(hi + [2099])), Con(K([0, 2048]))],
    ]
    com = [0, 1, 0, 0]
    msgs = [b"committee merge wide %d" % g for g in range(4)]
    sign_all(eng, reg, groups, msgs, dst)
    ks = M.KeySet(eng, reg.pks, n)
    try:
        ks.set_committees(coms)
        s0 = eng.keyset_committee_merge_stats()
        res = eng.keyset_committee_merge_checked_batch(ks, com, com_args(coms, com, groups, as_rows=True), msgs, dst)
        s1 = eng.keyset_committee_merge_stats()
        assert [len(r) for r in res[1]] == [263, 5, 263, 263]
        assert eng.keyset_committee_fast_aggregate_verify_batch(ks, com, res[1], msgs, res[0], dst) == b"\x0f"
        assert res == yardstick(eng, ks, n, coms, com, groups, msgs, dst)
    finally:
        ks.close()
    assert res[2] == [[True, True, True, True, False, True], [True, False, True], [True, False, True, False, True, False], [True, False, True]]
    assert check_model(oracle, coms, com, groups, res) == delta(s1, s0) == dict(zip(STATS, (3, 1, 5, 0)))


def tree_case(eng, W):
    """three collectors each aggregate a third of the signers of every group; what they hand out is what the merge takes"""
    com = [5, 3, 1, 4, 2, 0]
    signers = [W.clean[c] for c in com]
    msgs = [b"committee tree %d" % g for g in range(len(com))]
    parts = [[set(ps[k::3]) for ps in signers] for k in range(3)]       # (the committee of one: two collectors have nothing)
    entries = [sign_positions(eng, W, com, p, msgs) for p in parts]
    return com, signers, msgs, entries


def run_tree(e, ks, W, com, msgs, entries):
    collected = [e.keyset_committee_aggregate_checked_batch(ks, com, en, msgs, W.dst) for en in entries]
    groups = [[(col[1][g], col[0][64 * g:64 * g + 64]) for col in collected] for g in range(len(com))]
    return e.keyset_committee_merge_checked_batch(ks, com, groups, msgs, W.dst)


def test_the_tree_end_to_end_on_one_context(eng, oracle, M, W):
    com, signers, msgs, entries = tree_case(eng, W)
    G = len(com)
    weights = [[1000 + 7 * i for i in range(W.n)], [1 << (i % 40) for i in range(W.n)]]
    dst2 = b"COMMITTEE-MERGE-SECOND-DST"
    vb = synth.make_batch_gpu(eng, oracle, 100, dst2, pool=8, invalid_every=7, spot=2)

    def fresh():
        e = M.Engine(0)
        ks = W.keyset(M, e, False)
        ks.set_weights(weights)
        return e, ks

    e, ks = fresh()
    try:
        res = run_tree(e, ks, W, com, msgs, entries)
        assert res[3] == bytes(G) and res[2] == [[True] * 3] * 5 + [[True, False, False]]
        assert res[1] == [row_of(ps, len(W.coms[c])) for c, ps in zip(com, signers)]
        assert e.keyset_committee_merge_stats() == dict(zip(STATS, (G, 0, 0, 0)))
        everything = synth.bitmap_of([True] * G)
        assert e.keyset_committee_fast_aggregate_verify_batch(ks, com, res[1], msgs, res[0], W.dst) == everything
        assert e.keyset_committee_fast_aggregate_verify_batch_rlc(ks, com, res[1], msgs, res[0], W.dst, seed=bytes(range(32))) == everything
        got = e.keyset_committee_weight_batch(ks, com, res[1]).tolist()
        assert got == [[sum(col[W.coms[c][p]] for p in ps) for col in weights] for c, ps in zip(com, signers)]
        # the same call after a verify call under a second DST equals the call on a context of its own
        assert e.verify_batch(vb[0], vb[1], vb[2], dst2) == synth.bitmap_of(vb[3])
        again = run_tree(e, ks, W, com, msgs, entries)
        bcom, bgroups, bmsgs = boundary_case(eng, W, b" tree")           # ... and so does one that needs the fallback
        b_again = e.keyset_committee_merge_checked_batch(ks, bcom, com_args(W.coms, bcom, bgroups), bmsgs, W.dst)
    finally:
        ks.close(); e.close()
    e, ks = fresh()
    try:
        assert run_tree(e, ks, W, com, msgs, entries) == again == res
    finally:
        ks.close(); e.close()
    e, ks = fresh()
    try:
        assert e.keyset_committee_merge_checked_batch(ks, bcom, com_args(W.coms, bcom, bgroups), bmsgs, W.dst) == b_again
        assert e.keyset_committee_merge_stats() == BOUNDARY_STATS
    finally:
        ks.close(); e.close()


def test_argument_errors(eng, M, W):
    lib, ctx = eng._lib, eng._ctx
    u8, u32, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    dst = b"TEST"
    coms = [list(range(13)), list(range(8, 24))]                         # rows of 2 bytes
    groups = sign_all(eng, W.reg, [[Con([0, 1]), Con([12])], [Con([13])]], [b"a", b"bc"], dst)
    flat = [c for cs in groups for c in cs]
    good_rows = [3, 0, 0, 0x10, 0x20, 0]                                 # positions {0, 1}, {12} of committee 0; {5} of committee 1
    sg = np.frombuffer(b"".join(c.sig for c in flat), dtype=np.uint8)
    data = np.frombuffer(b"abc", dtype=np.uint8)
    out = np.zeros(128, dtype=np.uint8); sel = np.zeros(4, dtype=np.uint8); used = np.zeros(1, dtype=np.uint8); st = np.zeros(2, dtype=np.uint8)
    P = lambda a: a.ctypes.data_as(u8)
    keep = []

    def arr(v, t):
        a = np.array(v, dtype=t); keep.append(a)
        return a.ctypes.data_as({np.uint8: u8, np.uint32: u32, np.uint64: u64}[t])

    ks = M.KeySet(eng, W.reg.pks, W.n)
    bare = M.KeySet(eng, W.reg.pks, W.n)                                # a handle without a committee table
    ks.set_committees(coms)
    h = ks._h

    def call(c=ctx, k=h, cm=(0, 1), r=good_rows, ro=(0, 4, 6), s=P(sg), co=(0, 2, 3), m=P(data), mo=(0, 1, 3), so=(0, 2, 4), g=2, d=dst, dl=4, o=P(out), q=P(sel),
             u=P(used), t=P(st)):
        cm = arr(cm, np.uint32) if cm is not None else None
        r = arr(r, np.uint8) if r is not None else None
        ro, co, mo, so = (arr(x, np.uint64) if x is not None else None for x in (ro, co, mo, so))
        return lib.blsbn254_keyset_committee_merge_checked_batch(c, k, cm, r, ro, s, co, m, mo, so, ctypes.c_size_t(g), d, ctypes.c_size_t(dl), o, q, u, t)

    def untouched():
        return out.tobytes() == b"\x5a" * 128 and sel.tobytes() == b"\x5a" * 4 and used.tobytes() == b"\x5a" and st.tobytes() == b"\x5a" * 2

    def err():
        return lib.blsbn254_last_error(ctx)

    try:
        out[:] = 0x5a; sel[:] = 0x5a; used[:] = 0x5a; st[:] = 0x5a
        stats0 = eng.keyset_committee_merge_stats()
        eng.profile_enable(True); eng.profile_reset()                   # every kernel launch of this context is recorded from here on
        for name in ("c", "k", "cm", "r", "ro", "s", "co", "m", "mo", "so", "d", "o", "q", "u", "t"):
            assert call(**{name: None}) == E_ARG and untouched(), name
            assert name == "c" or b"NULL" in err(), name
        e2 = M.Engine(0)                                                # a key set that belongs to another context
        try:
            assert call(c=e2._ctx) == E_ARG and untouched() and b"another context" in lib.blsbn254_last_error(e2._ctx)
        finally:
            e2.close()
        assert call(k=bare._h) == E_ARG and b"no committees" in err()
        assert call(cm=(0, 2)) == E_ARG and b"group 1 names committee 2 of 2" in err()
        assert call(cm=(5, 1)) == E_ARG and b"group 0 names committee 5 of 2" in err()
        assert call(ro=(0, 4, 7)) == E_ARG and b"group 1: the contribution rows must be 1 x 2 bytes" in err()
        assert call(ro=(0, 2, 4)) == E_ARG and b"group 0: the contribution rows must be 2 x 2 bytes" in err()
        assert call(so=(0, 2, 3)) == E_ARG and b"group 1: the row must be 2 bytes" in err()
        assert call(so=(0, 3, 5)) == E_ARG and b"group 0: the row must be 2 bytes" in err()
        assert call(r=[3, 0, 0, 0x30, 0x20, 0]) == E_ARG and b"contribution 1 sets a bit past the last member" in err()
        assert call(r=[3, 0x80, 0, 0x10, 0x20, 0]) == E_ARG and b"contribution 0 sets a bit past the last member" in err()
        assert call(r=[3, 0, 0, 0x10, 0xff, 0xff]) == 0                  # 16 members: no padding bits
        out[:] = 0x5a; sel[:] = 0x5a; used[:] = 0x5a; st[:] = 0x5a
        eng.profile_reset()
        stats0 = eng.keyset_committee_merge_stats()
        for name, bad in (("co", (0, 3, 2)), ("ro", (0, 6, 4)), ("mo", (0, 2, 1)), ("so", (0, 4, 2))):
            assert call(**{name: bad}) == E_ARG and b"offsets decrease" in err(), name
        assert call(co=(0, 2, (1 << 23) + 3), ro=(0, 4, 6 + (1 << 24))) == E_ARG and b"2^23" in err()
        assert call(co=(0, 2, 1 << 23), ro=(0, 4, (1 << 30) + 2)) == E_ARG and b"2^30" in err()
        assert call(g=(1 << 22) + 1) == E_ARG and b"launch chunk" in err()
        assert lib.blsbn254_keyset_committee_merge_stats(ctx, None) == E_ARG
        assert lib.blsbn254_keyset_committee_merge_stats(None, (ctypes.c_uint64 * 4)()) == E_ARG
        assert call(g=0) == 0
        assert call(g=0, cm=None, r=None, ro=None, s=None, co=None, m=None, mo=None, so=None, o=None, q=None, u=None, t=None) == 0
        launched = eng.profile_read()
        eng.profile_enable(False); eng.profile_reset()
        assert untouched() and launched == {} and eng.keyset_committee_merge_stats() == stats0           # nothing was enqueued or counted
        assert call() == 0 and st.tobytes() == bytes(2) and used.tobytes() == b"\x07"          # after the errors, the context still serves
        want_sel = row_of({0, 1, 12}, 13) + row_of({5}, 16)
        assert sel.tobytes() == want_sel and out.tobytes()[64:] == flat[2].sig
        # offsets that do not start at 0: a leading row with padding bits, a leading signature and message bytes that are not
        # looked at, and a row offset of the outputs that is only a base
        first = out.tobytes()
        out[:] = 0x5a; sel[:] = 0x5a; used[:] = 0x5a
        lead_s = np.concatenate([np.zeros(64, dtype=np.uint8), sg])
        lead_m = np.frombuffer(b"??abc", dtype=np.uint8)
        assert call(r=[0xff, 0xff, 0xff] + good_rows, ro=(3, 7, 9), s=P(lead_s), co=(1, 3, 4), m=P(lead_m), mo=(2, 3, 5), so=(1000, 1002, 1004)) == 0
        assert st.tobytes() == bytes(2) and used.tobytes() == b"\x07" and sel.tobytes() == want_sel and out.tobytes() == first
        assert delta(eng.keyset_committee_merge_stats(), stats0) == dict(zip(STATS, (4, 0, 0, 0)))
        with pytest.raises(ValueError):
            eng.keyset_committee_merge_checked_batch(ks, [0], [[([13], flat[0].sig)]], [b"a"], dst)
        with pytest.raises(ValueError):
            eng.keyset_committee_merge_checked_batch(ks, [0], [[(b"\x01", flat[0].sig)]], [b"a"], dst)
        with pytest.raises(ValueError):
            eng.keyset_committee_merge_checked_batch(ks, [2], [[]], [b"a"], dst)
        with pytest.raises(ValueError):
            eng.keyset_committee_merge_checked_batch(ks, [0], [[]], [], dst)
        assert eng.keyset_committee_merge_checked_batch(ks, [], [], [], dst) == (b"", [], [], b"")
    finally:
        eng.profile_enable(False)
        ks.close(); bare.close()
