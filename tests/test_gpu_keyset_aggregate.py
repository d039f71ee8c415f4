"""GPU tests (MI355X) of the checked signature aggregation over a registered key set (blsbn254_keyset_aggregate_checked_batch):
honest groups, entries left out without the fallback, one wrong signature among honest neighbours, cancelling errors, the
short outcomes, launch boundaries, other call families on the same context, the argument errors.  Expected values never come
from the call under test: the oracle (aggregate_sigs, fast_aggregate_verify, g1_add / g1_mul), known secret keys, or the
parent's entry points."""
import ctypes
import random

import numpy as np
import pytest

from tests import synth
from tests.gpu_support import eng, M
from tests.helpers import IDENT1, row_of
from tests.keyset_support import Committee, delta, good_keys, sign_sets, ST_SHORT
from tests.threshold_support import checked_flow

pytestmark = pytest.mark.gpu
R = synth.R
E_ARG = -1
u8 = ctypes.POINTER(ctypes.c_uint8)
u32 = ctypes.POINTER(ctypes.c_uint32)
u64 = ctypes.POINTER(ctypes.c_uint64)


def agg(oracle, entries, kept):
    return oracle.aggregate_sigs(b"".join(entries[i] for i in sorted(kept)), len(kept)) if kept else IDENT1


def split(out, rows, com):
    rb = (com.n + 7) // 8
    return [out[64 * g:64 * g + 64] for g in range(len(out) // 64)], [rows[rb * g:rb * g + rb] for g in range(len(rows) // rb)]


def check_groups(oracle, com, entries, kept, msgs, res, dst, honest_sums=True):
    """res of the call against the expected kept sets (None: a short group)"""
    sigs, rows = split(res[0], res[1], com)
    assert list(res[2]) == [ST_SHORT if k is None else 0 for k in kept]
    for g, k in enumerate(kept):
        if k is None:
            assert sigs[g] == IDENT1 and rows[g] == bytes(len(rows[g])), g
            continue
        assert rows[g] == row_of(k, com.n), g
        if honest_sums:
            assert sigs[g] == agg(oracle, entries[g], k), g
        assert oracle.fast_aggregate_verify(com.gather(k), len(k), msgs[g], sigs[g], dst), g


@pytest.mark.parametrize("n", [1, 33, 70])
def test_all_honest(eng, oracle, M, n):
    dst = M.DEFAULT_DST
    rnd = random.Random(300 + n)
    com = Committee(eng, n, 30 + n)
    good = good_keys(com)
    sizes = sorted({1, min(2, len(good)), max(1, len(good) // 2), len(good)})
    sets = [set(rnd.sample(good, s)) for s in sizes] + [{good[0]}, {good[-1]}]
    assert not any(com.at and {com.at["p"], com.at["negp"]} == s for s in sets)
    msgs = [b"aggregate honest %d/%d" % (n, g) for g in range(len(sets))]
    entries = sign_sets(eng, com, sets, msgs, dst)
    assert entries[0][min(sets[0])] == oracle.sign(com.sk[min(sets[0])], msgs[0], dst)
    ks = M.KeySet(eng, com.pks, n)
    try:
        s0 = eng.keyset_aggregate_stats()
        res = eng.keyset_aggregate_checked_batch(ks, [list(e.items())[::-1] for e in entries], msgs, dst)      # the wrapper sorts
        s1 = eng.keyset_aggregate_stats()
        assert eng.keyset_aggregate_checked_batch(ks, entries, msgs, dst) == res                              # dicts too
        check_groups(oracle, com, entries, sets, msgs, res, dst)
        assert eng.keyset_fast_aggregate_verify_batch(ks, res[1], msgs, res[0], dst) == synth.bitmap_of([True] * len(sets))
    finally:
        ks.close()
    assert delta(s1, s0) == {"optimistic_groups": len(sets), "fallback_groups": 0, "verified_signatures": 0, "short_groups": 0}


@pytest.mark.parametrize("n", [33, 70])
def test_left_out_without_fallback(eng, oracle, M, n):
    dst = M.DEFAULT_DST
    com = Committee(eng, n, 40 + n)
    at, good = com.at, good_keys(com)
    honest = set(good[::3])
    rest = [i for i in good if i not in honest]
    special = {at["ident"], at["off"], at["undec"], at["nonsub"]}
    sets = [honest | set(rest[:3]) | special, honest, set(rest[:3]) | special]
    msgs = [b"left out %d/%d" % (n, g) for g in range(3)]
    entries = sign_sets(eng, com, sets, msgs, dst)
    for g in (0, 2):
        a, b, c = rest[:3]
        entries[g][a] = b"\xff" * 32 + entries[g][a][32:]                          # does not decode
        entries[g][b] = entries[g][b][:63] + bytes([entries[g][b][63] ^ 1])        # off the curve
        entries[g][c] = IDENT1
    ks = M.KeySet(eng, com.pks, n)
    try:
        s0 = eng.keyset_aggregate_stats()
        res = eng.keyset_aggregate_checked_batch(ks, entries, msgs, dst)
        s1 = eng.keyset_aggregate_stats()
    finally:
        ks.close()
    check_groups(oracle, com, entries, [honest, honest, None], msgs, res, dst)
    assert delta(s1, s0) == {"optimistic_groups": 2, "fallback_groups": 0, "verified_signatures": 0, "short_groups": 1}


def test_one_wrong_signature(eng, oracle, M):
    dst = M.DEFAULT_DST
    n = 70
    rnd = random.Random(51)
    com = Committee(eng, n, 51)
    good = [i for i in good_keys(com) if i != com.at["negp"]]
    sets = [set(rnd.sample(good, s)) for s in (5, 1, 12, 30, 2)]
    bad_g, bad_i = 2, sorted(sets[2])[4]
    msgs = [b"one wrong %d" % g for g in range(5)]
    entries = sign_sets(eng, com, sets, msgs, dst, sk=lambda g, i: com.sk[i] + 1 if (g, i) == (bad_g, bad_i) else None)
    spare = next(i for i in good if i not in sets[bad_g])
    entries[bad_g][spare] = IDENT1                                                 # a non-candidate: not verified, not counted
    kept = [set(s) for s in sets]
    kept[bad_g].discard(bad_i)
    ks = M.KeySet(eng, com.pks, n)
    try:
        s0 = eng.keyset_aggregate_stats()
        res = eng.keyset_aggregate_checked_batch(ks, entries, msgs, dst)
        s1 = eng.keyset_aggregate_stats()
        others = [g for g in range(5) if g != bad_g]
        alone = eng.keyset_aggregate_checked_batch(ks, [entries[g] for g in others], [msgs[g] for g in others], dst)
        s2 = eng.keyset_aggregate_stats()
    finally:
        ks.close()
    check_groups(oracle, com, entries, kept, msgs, res, dst)
    assert delta(s1, s0) == {"optimistic_groups": 4, "fallback_groups": 1, "verified_signatures": len(sets[bad_g]), "short_groups": 0}
    assert delta(s2, s1) == {"optimistic_groups": 4, "fallback_groups": 0, "verified_signatures": 0, "short_groups": 0}
    sg, rw = split(res[0], res[1], com)
    sa, ra = split(alone[0], alone[1], com)
    assert [sg[g] for g in others] == sa and [rw[g] for g in others] == ra and alone[2] == bytes(4)


def test_cancelling_errors(eng, oracle, M):
    dst = M.DEFAULT_DST
    n = 33
    com = Committee(eng, n, 61)
    good = good_keys(com)
    sets = [set(good[:4]), set(good[4:6])]
    msgs = [b"cancelling 0", b"cancelling 1"]
    honest = sign_sets(eng, com, sets, msgs, dst)
    entries = [dict(e) for e in honest]
    G = oracle.g1_generator()
    d = random.Random(62).randrange(1, R)
    a, b = sorted(sets[0])[:2]
    entries[0][a] = oracle.g1_add(honest[0][a], oracle.g1_mul(G, d))
    entries[0][b] = oracle.g1_add(honest[0][b], oracle.g1_mul(G, R - d))
    ks = M.KeySet(eng, com.pks, n)
    try:
        pk = b"".join(com.keys[i] for i in (a, b))
        assert eng.verify_batch(pk, [msgs[0]] * 2, entries[0][a] + entries[0][b], dst) == b"\x00"         # neither verifies on its own
        s0 = eng.keyset_aggregate_stats()
        res = eng.keyset_aggregate_checked_batch(ks, entries, msgs, dst)
        s1 = eng.keyset_aggregate_stats()
    finally:
        ks.close()
    check_groups(oracle, com, honest, sets, msgs, res, dst)                          # both bits, the bytes of the honest sum
    assert delta(s1, s0) == {"optimistic_groups": 2, "fallback_groups": 0, "verified_signatures": 0, "short_groups": 0}


def test_short_groups(eng, oracle, M):
    dst = M.DEFAULT_DST
    n = 70
    com = Committee(eng, n, 71)
    at, good = com.at, good_keys(com)
    plain = [i for i in good if i not in (at["p"], at["negp"], at["dup_a"], at["dup_b"])]
    sets = [set(plain[:3]), set(), {plain[3], at["off"]}, {at["p"], at["negp"]}, {at["p"]}, {at["dup_a"], at["dup_b"]}, set(plain[4:9])]
    msgs = [b"short %d" % g for g in range(len(sets))]
    entries = sign_sets(eng, com, sets, msgs, dst, sk=lambda g, i: com.sk[i] + 7 if g == 0 else None)     # group 0: every signature wrong
    entries[2][plain[3]] = IDENT1                                                  # group 2: only non-candidates
    ks = M.KeySet(eng, com.pks, n)
    try:
        s0 = eng.keyset_aggregate_stats()
        res = eng.keyset_aggregate_checked_batch(ks, entries, msgs, dst)
        s1 = eng.keyset_aggregate_stats()
        pn = sorted(sets[3])
        each = eng.verify_batch(b"".join(com.keys[i] for i in pn), [msgs[3]] * 2, b"".join(entries[3][i] for i in pn), dst)
    finally:
        ks.close()
    assert each == b"\x03"                                                          # P and -P: both signatures verify on their own
    check_groups(oracle, com, entries, [None, None, None, None, sets[4], sets[5], sets[6]], msgs, res, dst)
    assert delta(s1, s0) == {"optimistic_groups": 3, "fallback_groups": 2, "verified_signatures": 3 + 2, "short_groups": 4}


def boundary_case(eng, com, dst):
    rnd = random.Random(81)
    good = [i for i in good_keys(com) if i != com.at["negp"]]
    sets = [set(rnd.sample(good, s)) for s in (20, 3, 0, 11, 1, 9)]
    msgs = [b"launch boundaries %d" % g for g in range(len(sets))]
    wrong = (0, sorted(sets[0])[13])
    entries = sign_sets(eng, com, sets, msgs, dst, sk=lambda g, i: com.sk[i] + 1 if (g, i) == wrong else None)
    entries[3][com.at["off"]] = entries[3][min(sets[3])]
    kept = [set(s) if s else None for s in sets]
    kept[0].discard(wrong[1])
    return entries, kept, msgs


def test_launch_boundaries(eng, oracle, M, monkeypatch):
    dst = M.DEFAULT_DST
    n = 70
    com = Committee(eng, n, 81)
    entries, kept, msgs = boundary_case(eng, com, dst)
    results = []
    for chunk in (None, "8", "16"):                                     # cuts inside a group's entries, between groups, inside a group's row
        with monkeypatch.context() as mp:
            if chunk:
                mp.setenv("BLSBN254_CHUNK_LANES", chunk)
            e = M.Engine(0)
            try:
                ks = M.KeySet(e, com.pks, n)
                results.append(e.keyset_aggregate_checked_batch(ks, entries, msgs, dst))
                assert e.keyset_aggregate_stats() == {"optimistic_groups": 4, "fallback_groups": 1, "verified_signatures": 20, "short_groups": 1}
                ks.close()
            finally:
                e.close()
    check_groups(oracle, com, entries, kept, msgs, results[0], dst)
    assert results[1] == results[0] and results[2] == results[0]


def test_other_call_families_on_one_context(eng, oracle, M):
    dst, dst2 = M.DEFAULT_DST, b"KEYSET-AGGREGATE-SECOND-DST"
    coms = [Committee(eng, 70, 91), Committee(eng, 33, 92)]
    entries, kept, msgs = boundary_case(eng, coms[0], dst)              # needs the fallback
    good1 = good_keys(coms[1])
    sets1 = [set(good1[:5]), set(good1[3:20]), {good1[-1]}]
    msgs1 = [b"second set %d" % g for g in range(3)]
    entries1 = sign_sets(eng, coms[1], sets1, msgs1, dst2)              # all honest, another tag
    vb = synth.make_batch_gpu(eng, oracle, 300, dst, pool=20, invalid_every=7, spot=2)
    deal = checked_flow(eng, 8, 4, 93, dst).args()
    fav_rows = [row_of(k, 70) for k in kept if k]
    fav_msgs = [m for m, k in zip(msgs, kept) if k]
    fav_sigs = b"".join(agg(oracle, entries[g], k) for g, k in enumerate(kept) if k)
    steps = [
        lambda e, k: e.keyset_aggregate_checked_batch(k[0], entries, msgs, dst),
        lambda e, k: e.keyset_aggregate_checked_batch(k[1], entries1, msgs1, dst2),
        lambda e, k: e.verify_batch(vb[0], vb[1], vb[2], dst),
        lambda e, k: e.keyset_aggregate_checked_batch(k[0], entries, msgs, dst),
        lambda e, k: e.threshold_combine_checked_batch(*deal),
        lambda e, k: e.keyset_fast_aggregate_verify_batch(k[0], fav_rows, fav_msgs, fav_sigs, dst),
        lambda e, k: e.keyset_aggregate_checked_batch(k[1], entries1, msgs1, dst2),
        lambda e, k: e.keyset_aggregate_checked_batch(k[0], entries, msgs, dst),
    ]

    def run(which):
        e = M.Engine(0)
        try:
            k = [M.KeySet(e, c.pks, c.n) for c in coms]
            try:
                return [steps[j](e, k) for j in which], e.keyset_aggregate_stats()
            finally:
                for h in k:
                    h.close()
        finally:
            e.close()

    fresh = [run([j])[0][0] for j in range(len(steps))]
    check_groups(oracle, coms[0], entries, kept, msgs, fresh[0], dst)
    check_groups(oracle, coms[1], entries1, sets1, msgs1, fresh[1], dst2)
    assert fresh[2] == synth.bitmap_of(vb[3]) and fresh[5] == synth.bitmap_of([True] * len(fav_rows))
    got, stats = run(range(len(steps)))
    for j, (a, b) in enumerate(zip(got, fresh)):
        assert a == b, "step %d differs from the same call on a context of its own" % j
    assert stats == {"optimistic_groups": 3 * 4 + 2 * 3, "fallback_groups": 3, "verified_signatures": 60, "short_groups": 3}


def test_argument_errors(eng, M):
    lib, ctx = eng._lib, eng._ctx
    dst = b"TEST"
    n = 13
    com = Committee(eng, n, 95)
    sets = [{0, 1, 12}, {5}]
    msgs = [b"a", b"bc"]
    ent = sign_sets(eng, com, sets, msgs, dst)
    idx = np.array([0, 1, 12, 5], dtype=np.uint32)
    sg = np.frombuffer(b"".join(ent[g][i] for g in range(2) for i in sorted(sets[g])), dtype=np.uint8)
    data = np.frombuffer(b"abc", dtype=np.uint8)
    pks = np.frombuffer(com.pks, dtype=np.uint8)
    out = np.zeros(128, dtype=np.uint8); sel = np.zeros(4, dtype=np.uint8); st = np.zeros(2, dtype=np.uint8)
    P = lambda a: a.ctypes.data_as(u8)
    h = ctypes.c_void_p()
    assert lib.blsbn254_keyset_create(ctx, P(pks), ctypes.c_size_t(n), ctypes.byref(h)) == 0
    keep = []

    def arr(v, t):
        a = np.array(v, dtype=t); keep.append(a)
        return a.ctypes.data_as(u32 if t == np.uint32 else u64)

    def call(c=ctx, k=h, i=idx.ctypes.data_as(u32), s=P(sg), so=(0, 3, 4), m=P(data), mo=(0, 1, 3), g=2, d=dst, dl=4, o=P(out), r=P(sel), t=P(st)):
        so = arr(so, np.uint64) if so is not None else None
        mo = arr(mo, np.uint64) if mo is not None else None
        return lib.blsbn254_keyset_aggregate_checked_batch(c, k, i, s, so, m, mo, ctypes.c_size_t(g), d, ctypes.c_size_t(dl), o, r, t)

    def untouched():
        return out.tobytes() == b"\x5a" * 128 and sel.tobytes() == b"\x5a" * 4 and st.tobytes() == b"\x5a" * 2

    out[:] = 0x5a; sel[:] = 0x5a; st[:] = 0x5a
    for name in ("c", "k", "i", "s", "so", "m", "mo", "d", "o", "r", "t"):
        assert call(**{name: None}) == E_ARG and untouched(), name
    e2 = M.Engine(0)                                                    # a key set that belongs to another context
    try:
        assert call(c=e2._ctx) == E_ARG and untouched()
    finally:
        e2.close()
    assert call(so=(0, 3, 2)) == E_ARG and b"offsets decrease" in lib.blsbn254_last_error(ctx)
    assert call(mo=(0, 2, 1)) == E_ARG and b"offsets decrease" in lib.blsbn254_last_error(ctx)
    assert call(so=(0, 3, (1 << 23) + 1)) == E_ARG and b"2^23" in lib.blsbn254_last_error(ctx)
    assert call(i=arr([0, 1, 13, 5], np.uint32)) == E_ARG and b"names no key" in lib.blsbn254_last_error(ctx)
    assert call(i=arr([0, 1, 1, 5], np.uint32)) == E_ARG and b"strictly increase" in lib.blsbn254_last_error(ctx)
    assert call(i=arr([0, 12, 1, 5], np.uint32)) == E_ARG and b"group 0" in lib.blsbn254_last_error(ctx)
    assert call(g=(1 << 22) + 1) == E_ARG and b"launch chunk" in lib.blsbn254_last_error(ctx)
    assert lib.blsbn254_keyset_aggregate_stats(ctx, None) == E_ARG and lib.blsbn254_keyset_aggregate_stats(None, (ctypes.c_uint64 * 4)()) == E_ARG
    assert untouched()
    assert call(g=0) == 0 and call(g=0, i=None, s=None, so=None, m=None, mo=None, o=None, r=None, t=None) == 0 and untouched()
    assert call() == 0 and st.tobytes() == bytes(2)                     # after the errors, the context still serves
    assert sel.tobytes() == row_of(sets[0], n) + row_of(sets[1], n) and out.tobytes()[64:] == ent[1][5]
    # non-zero first offsets: one leading entry and group that are not looked at
    out[:] = 0x5a
    lead_i = arr([99, 0, 1, 12, 5], np.uint32)
    lead_s = np.concatenate([np.zeros(64, dtype=np.uint8), sg])
    lead_m = np.frombuffer(b"??abc", dtype=np.uint8)
    assert call(i=lead_i, s=P(lead_s), so=(1, 4, 5), m=P(lead_m), mo=(2, 3, 5)) == 0 and st.tobytes() == bytes(2)
    assert sel.tobytes() == row_of(sets[0], n) + row_of(sets[1], n) and out.tobytes()[64:] == ent[1][5]
    lib.blsbn254_keyset_destroy(h)
    ks = M.KeySet(eng, com.pks, n)
    try:
        with pytest.raises(ValueError):
            eng.keyset_aggregate_checked_batch(ks, [[(1, ent[0][1]), (1, ent[0][1])]], [b"a"], dst)
        with pytest.raises(ValueError):
            eng.keyset_aggregate_checked_batch(ks, [ent[0]], [], dst)
        assert eng.keyset_aggregate_checked_batch(ks, [], [], dst) == (b"", b"", b"")
    finally:
        ks.close()
