"""GPU tests (MI355X) of the checked merge of partial aggregates over a registered key set
(blsbn254_keyset_merge_checked_batch): honest disjoint contributions, contributions left out without the fallback, one bad group
among honest neighbours, cancelling errors, the short outcomes, launch boundaries, the order of a group's contributions, other
call families on the same context, rows of more than 64 words, the argument errors.  Expected values never come from the call
under test: the oracle (aggregate_sigs, fast_aggregate_verify, g1_add / g1_mul), known secret keys (a contribution's signature
is sign_batch under the sum of its keys' secrets), a sequential Python model of the selection, or the parent's
keyset_fast_aggregate_verify_batch."""
import ctypes
import random

import numpy as np
import pytest

from tests import synth
from tests.gpu_support import eng, M
from tests.helpers import IDENT1, row_of
from tests.keyset_support import as_args, chunks, Committee, Con, delta, expect, good_keys, sign_all, ST_SHORT, STATS

pytestmark = pytest.mark.gpu
R = synth.R
E_ARG = -1
u8 = ctypes.POINTER(ctypes.c_uint8)
u64 = ctypes.POINTER(ctypes.c_uint64)


def check_groups(oracle, com, groups, msgs, res, dst, kinds=None, gather=True):
    """res of the call against the model; returns the stats the call must have added"""
    rb = (com.n + 7) // 8
    tally = dict.fromkeys(STATS, 0)
    assert len(res[0]) == 64 * len(groups) and len(res[1]) == rb * len(groups) and len(res[2]) == len(groups) == len(res[3])
    for g, cs in enumerate(groups):
        used, union, fb, verified = expect(cs, kinds[g] if kinds else None)
        sig, row = res[0][64 * g:64 * g + 64], res[1][rb * g:rb * g + rb]
        tally["fallback_groups"] += fb; tally["verified_contributions"] += verified
        assert res[2][g] == used, g
        if union is None:
            assert res[3][g] == ST_SHORT and sig == IDENT1 and row == bytes(rb), g
            tally["short_groups"] += 1
            continue
        tally["optimistic_groups"] += not fb
        kept = [c.sig for c, u in zip(cs, used) if u]
        assert res[3][g] == 0 and row == row_of(union, com.n), g
        assert sig == oracle.aggregate_sigs(b"".join(kept), len(kept)), g
        if gather:
            assert oracle.fast_aggregate_verify(com.gather(union), len(union), msgs[g], sig, dst), g
    return tally


@pytest.mark.parametrize("n", [1, 33, 70])
def test_all_honest_and_disjoint(eng, oracle, M, n):
    dst = M.DEFAULT_DST
    rnd = random.Random(400 + n)
    com = Committee(eng, n, 130 + n)
    good = [i for i in good_keys(com) if i != com.at.get("negp")]
    rnd.shuffle(good)
    if n == 1:
        shapes = [[1]]
    else:
        shapes = [[1], [len(good)], [3, 1, 2, 5, 4, 6], [1, 1], [len(good) - 7, 7]]
    groups = [[Con(k) for k in chunks(good, s)] for s in shapes]
    msgs = [b"merge honest %d/%d" % (n, g) for g in range(len(groups))]
    sign_all(eng, com, groups, msgs, dst)
    one = sorted(groups[0][0].keys)[0]
    assert groups[0][0].sig == oracle.sign(com.sk[one], msgs[0], dst)
    ks = M.KeySet(eng, com.pks, n)
    try:
        s0 = eng.keyset_merge_stats()
        res = eng.keyset_merge_checked_batch(ks, as_args(groups), msgs, dst)
        s1 = eng.keyset_merge_stats()
        assert eng.keyset_merge_checked_batch(ks, as_args(groups, n), msgs, dst) == res                         # rows as bytes too
        assert eng.keyset_fast_aggregate_verify_batch(ks, res[1], msgs, res[0], dst) == synth.bitmap_of([True] * len(groups))
    finally:
        ks.close()
    assert all(all(u) for u in res[2]) and res[3] == bytes(len(groups))
    assert check_groups(oracle, com, groups, msgs, res, dst) == delta(s1, s0) == dict(zip(STATS, (len(groups), 0, 0, 0)))


@pytest.mark.parametrize("n", [33, 70])
def test_left_out_without_fallback(eng, oracle, M, n):
    dst = M.DEFAULT_DST
    com = Committee(eng, n, 140 + n)
    at = com.at
    good = [i for i in good_keys(com) if i != at["negp"]]
    A, B, X, Y, Z, V = chunks(good, [4, 3, 2, 2, 2, 2])

    def build():
        return [
            [Con(A), Con(A[2:] + X), Con(A), Con([], cand=False, good=False), Con(B)],                      # overlapping, duplicate, empty row
            [Con(A), Con(X), Con(Y), Con(Z), Con(B)],                                                       # signatures that are no candidates
            [Con(A), Con(X + [at["ident"]], cand=False), Con(Y + [at["off"]], cand=False), Con(Z + [at["undec"]], cand=False),
             Con(V + [at["nonsub"]], cand=False), Con(B)],                                                  # rows that select a key without KeyValidate
        ]
    groups = build()
    msgs = [b"merge left out %d/%d" % (n, g) for g in range(3)]
    sign_all(eng, com, groups, msgs, dst)
    s = groups[1]
    s[1].broken(IDENT1)
    s[2].broken(s[2].sig[:63] + bytes([s[2].sig[63] ^ 1]))                                                  # off the curve
    s[3].broken(b"\xff" * 32 + s[3].sig[32:])                                                               # does not decode
    ks = M.KeySet(eng, com.pks, n)
    try:
        s0 = eng.keyset_merge_stats()
        res = eng.keyset_merge_checked_batch(ks, as_args(groups), msgs, dst)
        s1 = eng.keyset_merge_stats()
    finally:
        ks.close()
    assert res[2] == [[True, False, False, False, True], [True, False, False, False, True], [True, False, False, False, False, True]]
    assert check_groups(oracle, com, groups, msgs, res, dst) == delta(s1, s0) == dict(zip(STATS, (3, 0, 0, 0)))


@pytest.mark.parametrize("bad", ["wrong_signature", "one_key_too_many"])
def test_one_bad_group_among_honest_neighbours(eng, oracle, M, bad):
    dst = M.DEFAULT_DST
    n = 70
    com = Committee(eng, n, 151)
    good = [i for i in good_keys(com) if i != com.at["negp"]]
    A, B, K, C2, D, extra = chunks(good, [5, 6, 4, 3, 2, 1])
    if bad == "wrong_signature":
        bad_con, late = Con(K, sk_delta=1, good=False), Con(K[-1:] + C2)
    else:
        bad_con, late = Con(K + extra, signed=K, good=False), Con(extra + C2)          # a correct signature of K under a row that claims one more key
    groups = [[Con(A), Con(B)], [Con(D)], [Con(A), bad_con, late, Con(D), Con([], cand=False)], [Con(B), Con(A + D), Con(D)], [Con(K)]]
    msgs = [b"merge one bad %d" % g for g in range(len(groups))]
    sign_all(eng, com, groups, msgs, dst)
    others = [g for g in range(len(groups)) if g != 2]
    ks = M.KeySet(eng, com.pks, n)
    try:
        assert eng.keyset_fast_aggregate_verify_batch(ks, [row_of(bad_con.keys, n), row_of(late.keys, n)], [msgs[2]] * 2, bad_con.sig + late.sig, dst) == b"\x02"
        s0 = eng.keyset_merge_stats()
        res = eng.keyset_merge_checked_batch(ks, as_args(groups), msgs, dst)
        s1 = eng.keyset_merge_stats()
        alone = eng.keyset_merge_checked_batch(ks, as_args([groups[g] for g in others]), [msgs[g] for g in others], dst)
        s2 = eng.keyset_merge_stats()
    finally:
        ks.close()
    assert res[2][2] == [True, False, True, True, False]                           # the bad one dropped, the later one that overlapped only it used
    assert check_groups(oracle, com, groups, msgs, res, dst) == delta(s1, s0) == dict(zip(STATS, (4, 1, 4, 0)))
    assert delta(s2, s1) == dict(zip(STATS, (4, 0, 0, 0)))
    rb = (n + 7) // 8
    assert b"".join(res[0][64 * g:64 * g + 64] for g in others) == alone[0] and b"".join(res[1][rb * g:rb * g + rb] for g in others) == alone[1]
    assert [res[2][g] for g in others] == alone[2] and alone[3] == bytes(4)


def test_cancelling_errors(eng, oracle, M):
    dst = M.DEFAULT_DST
    n = 33
    com = Committee(eng, n, 161)
    good = [i for i in good_keys(com) if i != com.at["negp"]]
    A, B, C = chunks(good, [3, 2, 4])
    groups = [[Con(A), Con(B), Con(C)], [Con(C)]]
    msgs = [b"merge cancelling 0", b"merge cancelling 1"]
    sign_all(eng, com, groups, msgs, dst)
    G = oracle.g1_generator()
    d = random.Random(162).randrange(1, R)
    a, b = groups[0][0], groups[0][1]
    a.sig = oracle.g1_add(a.sig, oracle.g1_mul(G, d)); a.good = False
    b.sig = oracle.g1_add(b.sig, oracle.g1_mul(G, R - d)); b.good = False
    ks = M.KeySet(eng, com.pks, n)
    try:
        assert eng.keyset_fast_aggregate_verify_batch(ks, [row_of(A, n), row_of(B, n)], [msgs[0]] * 2, a.sig + b.sig, dst) == b"\x00"   # neither verifies on its own
        s0 = eng.keyset_merge_stats()
        res = eng.keyset_merge_checked_batch(ks, as_args(groups), msgs, dst)
        s1 = eng.keyset_merge_stats()
    finally:
        ks.close()
    assert res[2] == [[True, True, True], [True]]
    assert check_groups(oracle, com, groups, msgs, res, dst, kinds=["cancel", None]) == delta(s1, s0) == dict(zip(STATS, (2, 0, 0, 0)))


def test_short_groups(eng, oracle, M):
    dst = M.DEFAULT_DST
    n = 70
    com = Committee(eng, n, 171)
    at = com.at
    good = [i for i in good_keys(com) if i not in (at["p"], at["negp"])]
    A, B, C = chunks(good, [3, 2, 4])
    groups = [
        [],                                                                          # no contributions
        [Con(A), Con([], cand=False), Con(B + [at["off"]], cand=False)],             # no candidate (the first signature becomes the identity below)
        [Con(A, sk_delta=3, good=False), Con(B, sk_delta=5, good=False)],            # every candidate fails
        [Con([at["p"]]), Con([at["negp"]])],                                         # each verifies, the kept keys are P and -P
        [Con(A), Con(B), Con(C)],
    ]
    msgs = [b"merge short %d" % g for g in range(len(groups))]
    sign_all(eng, com, groups, msgs, dst)
    groups[1][0].broken(IDENT1)
    ks = M.KeySet(eng, com.pks, n)
    try:
        pn = groups[3]
        assert eng.keyset_fast_aggregate_verify_batch(ks, [row_of(c.keys, n) for c in pn], [msgs[3]] * 2, pn[0].sig + pn[1].sig, dst) == b"\x03"
        s0 = eng.keyset_merge_stats()
        res = eng.keyset_merge_checked_batch(ks, as_args(groups), msgs, dst)
        s1 = eng.keyset_merge_stats()
        empty = eng.keyset_merge_checked_batch(ks, [[], []], msgs[:2], dst)             # a call without any contribution
        s2 = eng.keyset_merge_stats()
    finally:
        ks.close()
    assert empty == (IDENT1 * 2, bytes(2 * ((n + 7) // 8)), [[], []], bytes([ST_SHORT] * 2)) and delta(s2, s1) == dict(zip(STATS, (0, 0, 0, 2)))
    assert res[3] == bytes([ST_SHORT] * 4 + [0]) and res[2][:4] == [[], [False] * 3, [False] * 2, [False] * 2]
    assert check_groups(oracle, com, groups, msgs, res, dst, kinds=[None, None, None, "zero_sum", None]) == delta(s1, s0) == dict(zip(STATS, (1, 2, 4, 4)))


def boundary_case(eng, com, dst, tag=b""):
    """six groups with 0 to 6 contributions; group 0 needs the fallback, which then uses a contribution it had left out"""
    good = [i for i in good_keys(com) if i != com.at["negp"]]
    A, B, K, C2, D, E, F = chunks(good, [7, 5, 4, 3, 2, 6, 1])
    groups = [
        [Con(A), Con(K, sk_delta=1, good=False), Con(K[:1] + C2), Con(D), Con(A[:2]), Con(E + F)],
        [Con(B), Con(A), Con(B[:1] + E)],
        [],
        [Con(F), Con(E + [com.at["off"]], cand=False), Con(D), Con(K + C2)],
        [Con(E)],
        [Con(A + B), Con(K), Con(C2), Con(D), Con(E), Con(F)],
    ]
    msgs = [b"merge launch boundaries %d" % g + tag for g in range(len(groups))]
    return sign_all(eng, com, groups, msgs, dst), msgs


BOUNDARY_STATS = dict(zip(STATS, (4, 1, 6, 1)))


def test_launch_boundaries(eng, oracle, M, monkeypatch):
    dst = M.DEFAULT_DST
    n = 70
    com = Committee(eng, n, 181)
    groups, msgs = boundary_case(eng, com, dst)
    results = []
    for chunk in (None, "8", "16"):                                     # cuts inside a group's contributions and between groups; a group per select launch
        with monkeypatch.context() as mp:
            if chunk:
                mp.setenv("BLSBN254_CHUNK_LANES", chunk)
            e = M.Engine(0)
            try:
                ks = M.KeySet(e, com.pks, n)
                results.append(e.keyset_merge_checked_batch(ks, as_args(groups), msgs, dst))
                assert e.keyset_merge_stats() == BOUNDARY_STATS
                ks.close()
            finally:
                e.close()
    assert check_groups(oracle, com, groups, msgs, results[0], dst) == BOUNDARY_STATS
    assert results[0][2][0] == [True, False, True, True, False, True]
    assert results[1] == results[0] and results[2] == results[0]


def test_order_matters(eng, oracle, M):
    dst = M.DEFAULT_DST
    n = 33
    com = Committee(eng, n, 191)
    good = [i for i in good_keys(com) if i != com.at["negp"]]
    A, B, C = chunks(good, [4, 3, 5])
    a, ab, bc, c = Con(A), Con(A[-1:] + B), Con(B[-1:] + C), Con(C)
    groups = [[a, ab, bc, c], [c, bc, ab, a], [ab, a, c, bc], [bc, ab, a, c]]
    msgs = [b"merge order"] * 4
    sign_all(eng, com, [[a, ab, bc, c]], msgs, dst)
    ks = M.KeySet(eng, com.pks, n)
    try:
        res = eng.keyset_merge_checked_batch(ks, as_args(groups), msgs, dst)
    finally:
        ks.close()
    assert res[2] == [[True, False, True, False], [True, False, True, False], [True, False, True, False], [True, False, True, False]]
    rb = (n + 7) // 8
    rows = [res[1][rb * g:rb * g + rb] for g in range(4)]
    assert rows == [row_of(A + B[-1:] + C, n), row_of(C + A[-1:] + B, n), row_of(A[-1:] + B + C, n), row_of(B[-1:] + C + A, n)]
    assert rows[0] != rows[1] and rows[2] == rows[1] and rows[3] == rows[0]                 # two outcomes, by the order alone
    assert check_groups(oracle, com, groups, msgs, res, dst)["optimistic_groups"] == 4


def test_more_than_64_words(eng, oracle, M):
    """a committee of 2100 keys: rows of 66 words (263 bytes), the union kept in the merged row.  Validity by the parent's
    keyset call; bytes by the oracle's aggregate and the model"""
    dst = M.DEFAULT_DST
    n = 2100
    com = Committee(eng, n, 201)
    at = com.at
    good = [i for i in good_keys(com) if i != at["negp"]]
    lo, mid, hi = [i for i in good if i < 700], [i for i in good if 700 <= i < 2040], [i for i in good if 2052 <= i < 2099]
    edge = [2040, 2047, 2048, 2051]                                      # lane 63's word and lane 0's second word
    groups = [
        [Con(lo), Con(mid), Con(edge), Con(hi), Con([2047, 2090]), Con([2099])],
        [Con(mid), Con(lo, sk_delta=1, good=False), Con([3 * k for k in range(10, 200)]), Con(edge[:2] + [at["undec"]], cand=False), Con(edge[2:]), Con([2048])],
        [Con([2099]), Con(hi + [2099]), Con([0, 2048])],
    ]
    msgs = [b"merge wide %d" % g for g in range(3)]
    sign_all(eng, com, groups, msgs, dst)
    ks = M.KeySet(eng, com.pks, n)
    try:
        s0 = eng.keyset_merge_stats()
        res = eng.keyset_merge_checked_batch(ks, as_args(groups, n), msgs, dst)
        s1 = eng.keyset_merge_stats()
        assert eng.keyset_fast_aggregate_verify_batch(ks, res[1], msgs, res[0], dst) == b"\x07"
    finally:
        ks.close()
    assert res[2] == [[True, True, True, True, False, True], [True, False, True, False, True, False], [True, False, True]]
    assert check_groups(oracle, com, groups, msgs, res, dst, gather=False) == delta(s1, s0) == dict(zip(STATS, (2, 1, 5, 0)))


def test_other_call_families_on_one_context(eng, oracle, M):
    dst, dst2 = M.DEFAULT_DST, b"KEYSET-MERGE-SECOND-DST"
    coms = [Committee(eng, 70, 211), Committee(eng, 33, 212)]
    groups, msgs = boundary_case(eng, coms[0], dst)                      # needs the fallback
    good1 = [i for i in good_keys(coms[1]) if i != coms[1].at["negp"]]
    groups1 = [[Con(k) for k in chunks(good1, s)] for s in ([5, 2], [1], [4, 4, 4])]
    msgs1 = [b"merge second set %d" % g for g in range(3)]
    sign_all(eng, coms[1], groups1, msgs1, dst2)                         # all honest, another tag
    sets = [set(good1[:5]), set(good1[3:9])]
    ka_msgs = [b"merge beside aggregate %d" % g for g in range(2)]
    singles = sign_all(eng, coms[1], [[Con([i]) for i in sorted(s)] for s in sets], ka_msgs, dst)
    entries = [{min(c.keys): c.sig for c in cs} for cs in singles]
    vb = synth.make_batch_gpu(eng, oracle, 300, dst, pool=20, invalid_every=7, spot=2)
    fav = [(row_of(c.keys, 70), msgs[g], c.sig) for g, cs in enumerate(groups) for c in cs[:1]]
    steps = [
        lambda e, k: e.keyset_merge_checked_batch(k[0], as_args(groups), msgs, dst),
        lambda e, k: e.keyset_merge_checked_batch(k[1], as_args(groups1), msgs1, dst2),
        lambda e, k: e.verify_batch(vb[0], vb[1], vb[2], dst),
        lambda e, k: e.keyset_merge_checked_batch(k[0], as_args(groups), msgs, dst),
        lambda e, k: e.keyset_aggregate_checked_batch(k[1], entries, ka_msgs, dst),
        lambda e, k: e.keyset_fast_aggregate_verify_batch(k[0], [f[0] for f in fav], [f[1] for f in fav], b"".join(f[2] for f in fav), dst),
        lambda e, k: e.keyset_merge_checked_batch(k[1], as_args(groups1), msgs1, dst2),
        lambda e, k: e.keyset_merge_checked_batch(k[0], as_args(groups), msgs, dst),
    ]

    def run(which):
        e = M.Engine(0)
        try:
            k = [M.KeySet(e, c.pks, c.n) for c in coms]
            try:
                return [steps[j](e, k) for j in which], e.keyset_merge_stats(), e.keyset_aggregate_stats(), e.keyset_stats()
            finally:
                for h in k:
                    h.close()
        finally:
            e.close()

    fresh = [run([j])[0][0] for j in range(len(steps))]
    assert check_groups(oracle, coms[0], groups, msgs, fresh[0], dst) == BOUNDARY_STATS
    assert check_groups(oracle, coms[1], groups1, msgs1, fresh[1], dst2)["optimistic_groups"] == 3
    assert fresh[2] == synth.bitmap_of(vb[3]) and fresh[5] == synth.bitmap_of([True] * len(fav)) and fresh[4][2] == bytes(2)
    got, merge_stats, agg_stats, ks_stats = run(range(len(steps)))
    for j, (a, b) in enumerate(zip(got, fresh)):
        assert a == b, "step %d differs from the same call on a context of its own" % j
    assert merge_stats == {k: 3 * v + (6 if k == "optimistic_groups" else 0) for k, v in BOUNDARY_STATS.items()}
    # the merge calls count in neither of the other two families' counters
    assert agg_stats["optimistic_groups"] == 2 and agg_stats["fallback_groups"] == 0 and ks_stats["groups"] == len(fav) and ks_stats["key_sets"] == 2


def test_argument_errors(eng, M):
    lib, ctx = eng._lib, eng._ctx
    dst = b"TEST"
    n = 13
    com = Committee(eng, n, 221)
    groups = sign_all(eng, com, [[Con([0, 1]), Con([12])], [Con([5])]], [b"a", b"bc"], dst)
    flat = [c for cs in groups for c in cs]
    rows = np.frombuffer(b"".join(row_of(c.keys, n) for c in flat), dtype=np.uint8)
    sg = np.frombuffer(b"".join(c.sig for c in flat), dtype=np.uint8)
    data = np.frombuffer(b"abc", dtype=np.uint8)
    pks = np.frombuffer(com.pks, dtype=np.uint8)
    out = np.zeros(128, dtype=np.uint8); sel = np.zeros(4, dtype=np.uint8); used = np.zeros(1, dtype=np.uint8); st = np.zeros(2, dtype=np.uint8)
    P = lambda a: a.ctypes.data_as(u8)
    h = ctypes.c_void_p()
    assert lib.blsbn254_keyset_create(ctx, P(pks), ctypes.c_size_t(n), ctypes.byref(h)) == 0
    keep = []

    def arr(v, t=np.uint64):
        a = np.array(v, dtype=t); keep.append(a)
        return a.ctypes.data_as(u8 if t == np.uint8 else u64)

    def call(c=ctx, k=h, r=P(rows), s=P(sg), co=(0, 2, 3), m=P(data), mo=(0, 1, 3), g=2, d=dst, dl=4, o=P(out), q=P(sel), u=P(used), t=P(st)):
        co = arr(co) if co is not None else None
        mo = arr(mo) if mo is not None else None
        return lib.blsbn254_keyset_merge_checked_batch(c, k, r, s, co, m, mo, ctypes.c_size_t(g), d, ctypes.c_size_t(dl), o, q, u, t)

    def untouched():
        return out.tobytes() == b"\x5a" * 128 and sel.tobytes() == b"\x5a" * 4 and used.tobytes() == b"\x5a" and st.tobytes() == b"\x5a" * 2

    def err():
        return lib.blsbn254_last_error(ctx)

    out[:] = 0x5a; sel[:] = 0x5a; used[:] = 0x5a; st[:] = 0x5a
    for name in ("c", "k", "r", "s", "co", "m", "mo", "d", "o", "q", "u", "t"):
        assert call(**{name: None}) == E_ARG and untouched(), name
        assert name == "c" or b"NULL" in err(), name
    assert call(u=None) == E_ARG and b"NULL" in err()
    e2 = M.Engine(0)                                                    # a key set that belongs to another context
    try:
        assert call(c=e2._ctx) == E_ARG and untouched() and b"another context" in lib.blsbn254_last_error(e2._ctx)
    finally:
        e2.close()
    assert call(co=(0, 3, 2)) == E_ARG and b"offsets decrease" in err()
    assert call(mo=(0, 2, 1)) == E_ARG and b"offsets decrease" in err()
    assert call(co=(0, 3, (1 << 23) + 1)) == E_ARG and b"2^23" in err()
    assert call(g=(1 << 22) + 1) == E_ARG and b"launch chunk" in err()
    assert call(r=arr([3, 0, 0, 0x20, 0x20, 0], np.uint8)) == E_ARG and b"contribution 1 sets a bit past the last key" in err()
    assert call(r=arr([3, 0, 0, 0x10, 0x20, 0x80], np.uint8)) == E_ARG and b"contribution 2 sets a bit past the last key" in err()
    # more than 2^30 bytes of rows needs rows of more than 128 bytes for at most 2^23 contributions: the limit fires before a row is read
    wide = Committee(eng, 1040, 222, special=False)
    hw = ctypes.c_void_p()
    assert lib.blsbn254_keyset_create(ctx, P(np.frombuffer(wide.pks, dtype=np.uint8)), ctypes.c_size_t(1040), ctypes.byref(hw)) == 0
    assert call(k=hw, co=(0, 1 << 22, 1 << 23)) == E_ARG and b"2^30" in err()
    lib.blsbn254_keyset_destroy(hw)
    assert lib.blsbn254_keyset_merge_stats(ctx, None) == E_ARG and lib.blsbn254_keyset_merge_stats(None, (ctypes.c_uint64 * 4)()) == E_ARG
    assert untouched()
    s0 = eng.keyset_merge_stats()
    assert call(g=0) == 0 and call(g=0, r=None, s=None, co=None, m=None, mo=None, o=None, q=None, u=None, t=None) == 0 and untouched()
    assert call() == 0 and st.tobytes() == bytes(2) and used.tobytes() == b"\x07"          # after the errors, the context still serves
    want_sel = row_of({0, 1, 12}, n) + row_of({5}, n)
    assert sel.tobytes() == want_sel and out.tobytes()[64:] == flat[2].sig
    # non-zero first offsets: one leading contribution and message that are not looked at (the leading row has a padding bit)
    out[:] = 0x5a; used[:] = 0x5a
    lead_r = np.concatenate([np.array([0xff, 0xff], dtype=np.uint8), rows])
    lead_s = np.concatenate([np.zeros(64, dtype=np.uint8), sg])
    lead_m = np.frombuffer(b"??abc", dtype=np.uint8)
    assert call(r=P(lead_r), s=P(lead_s), co=(1, 3, 4), m=P(lead_m), mo=(2, 3, 5)) == 0 and st.tobytes() == bytes(2) and used.tobytes() == b"\x07"
    assert sel.tobytes() == want_sel and out.tobytes()[64:] == flat[2].sig
    assert delta(eng.keyset_merge_stats(), s0) == dict(zip(STATS, (4, 0, 0, 0)))
    lib.blsbn254_keyset_destroy(h)
    ks = M.KeySet(eng, com.pks, n)
    try:
        with pytest.raises(ValueError):
            eng.keyset_merge_checked_batch(ks, [[([13], flat[0].sig)]], [b"a"], dst)
        with pytest.raises(ValueError):
            eng.keyset_merge_checked_batch(ks, [[(b"\x01", flat[0].sig)]], [b"a"], dst)
        with pytest.raises(ValueError):
            eng.keyset_merge_checked_batch(ks, [[]], [], dst)
        assert eng.keyset_merge_checked_batch(ks, [], [], dst) == (b"", b"", [], b"")
    finally:
        ks.close()
