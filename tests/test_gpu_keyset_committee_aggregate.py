"""GPU tests (MI355X) of the checked signature aggregation per committee of a registered key set
(blsbn254_keyset_committee_aggregate_checked_batch).  The yardstick throughout is the EXISTING full-width call
Engine.keyset_aggregate_checked_batch on the entries translated to registry indices, on the same handle: signatures and statuses
byte for byte, the committee rows against the full-width rows read through the member lists.  One small committee is also
checked against the oracle, and every status-0 group against the committee verify."""
import ctypes
import random

import numpy as np
import pytest

import blsbn254_loader
from tests import synth
from tests.gpu_support import eng, fresh_engine, M
from tests.helpers import bits_of, IDENT1, row_of
from tests.keyset_support import compact, delta, sign_positions, sign_sets, ST_SHORT, World

pytestmark = pytest.mark.gpu
E_ARG = -1
R = synth.R
_M = blsbn254_loader.load()
_M.Engine.keyset_committee_aggregate_checked_batch          # the feature is there, or this module does not import
ZERO = {"optimistic_groups": 0, "fallback_groups": 0, "verified_signatures": 0, "short_groups": 0}


@pytest.fixture(scope="module")
def W(eng, M):
    return World(eng, M)


@pytest.fixture(scope="module")
def handles(eng, M, W):
    hs = {False: W.keyset(M, eng, False), True: W.keyset(M, eng, True)}
    yield hs
    for ks in hs.values():
        ks.close()


def yardstick(e, ks, W, com, entries, msgs, coms=None):
    """the full-width call on the translated entries (the wrapper re-sorts them by registry index), its rows read through the
    member lists"""
    coms = coms or W.coms
    out, wide, st = e.keyset_aggregate_checked_batch(ks, [{coms[c][p]: s for p, s in es.items()} for c, es in zip(com, entries)], msgs, W.dst)
    rbw = (W.n + 7) // 8
    return out, [compact(coms[c], wide[rbw * g:rbw * g + rbw]) for g, c in enumerate(com)], st


def signers(W, c, rows_g):
    return {W.coms[c][j] for j in range(len(W.coms[c])) if (rows_g[j >> 3] >> (j & 7)) & 1}


def honest_case(W):
    rnd = random.Random(5)
    groups = []
    for c, mem in enumerate(W.coms):
        s, clean = len(mem), W.clean[c]
        groups += [(c, set()), (c, {clean[0]}), (c, set(rnd.sample(clean, min(len(clean), s // 2)))), (c, set(rnd.sample(clean, min(len(clean), s // 2 + 1)))),
                   (c, set(range(s)))]
    rnd.shuffle(groups)
    com = [c for c, _ in groups]
    assert sum(1 for a, b in zip(com, com[1:]) if a != b) > len(com) // 2          # the caller's order interleaves the committees
    return com, [ps for _, ps in groups], [b"committee aggregate %d" % g for g in range(len(groups))]


@pytest.mark.parametrize("checked", [False, True])
def test_all_honest(eng, oracle, W, handles, checked):
    ks = handles[checked]
    com, pos_sets, msgs = honest_case(W)
    G = len(com)
    # (the full groups of committee 4 carry entries on its bad keys too: left out, no fallback; a lone P or -P is fine)
    entries = sign_positions(eng, W, com, pos_sets, msgs)
    others0 = (eng.keyset_stats(), eng.keyset_aggregate_stats(), eng.keyset_committee_stats())
    s0 = eng.keyset_committee_aggregate_stats()
    res = eng.keyset_committee_aggregate_checked_batch(ks, com, [list(e.items())[::-1] for e in entries], msgs, W.dst)       # the wrapper sorts
    s1 = eng.keyset_committee_aggregate_stats()
    assert (eng.keyset_stats(), eng.keyset_aggregate_stats(), eng.keyset_committee_stats()) == others0      # the siblings' counters are left alone
    assert eng.keyset_committee_aggregate_checked_batch(ks, com, entries, msgs, W.dst) == res               # dicts too
    y0 = eng.keyset_aggregate_stats()
    want = yardstick(eng, ks, W, com, entries, msgs)
    y1 = eng.keyset_aggregate_stats()
    assert res[2] == want[2] and res[0] == want[0] and res[1] == want[1]
    assert [len(r) for r in res[1]] == [(len(W.coms[c]) + 7) // 8 for c in com]
    assert list(res[2]) == [ST_SHORT if not ps else 0 for ps in pos_sets]
    empty = sum(1 for ps in pos_sets if not ps)                          # 7: one per committee, and "half" of the committee of one
    assert empty == 7
    assert delta(s1, s0) == delta(y1, y0) == {"optimistic_groups": G - empty, "fallback_groups": 0, "verified_signatures": 0, "short_groups": empty}
    excluded = W.reg.unsignable | {W.reg.at["ident"]} | ({12} if checked else set())
    for g, (c, ps) in enumerate(zip(com, pos_sets)):
        assert signers(W, c, res[1][g]) == {W.coms[c][p] for p in ps} - excluded, g
        if not ps:
            assert res[0][64 * g:64 * g + 64] == IDENT1 and res[1][g] == bytes(len(res[1][g]))
    # the committee verify accepts exactly the status-0 groups
    bits = bits_of(eng.keyset_committee_fast_aggregate_verify_batch(ks, com, res[1], msgs, res[0], W.dst), G)
    assert [bool(b) for b in bits] == [s == 0 for s in res[2]]
    # against the oracle, on the groups of the 31-member committee listed ascending and the 33-member one listed descending
    for g in [g for g in range(G) if com[g] in (1, 3) and pos_sets[g]]:
        keys = sorted(W.coms[com[g]][p] for p in pos_sets[g])
        by_key = {W.coms[com[g]][p]: s for p, s in entries[g].items()}
        sig = res[0][64 * g:64 * g + 64]
        assert sig == oracle.aggregate_sigs(b"".join(by_key[i] for i in keys), len(keys)), g
        assert oracle.fast_aggregate_verify(W.reg.gather(keys), len(keys), msgs[g], sig, W.dst), g


@pytest.mark.parametrize("checked", [False, True])
def test_left_out_without_fallback(eng, W, handles, checked):
    ks = handles[checked]
    at = W.reg.at
    honest4 = set(W.clean[4][::3])
    bad4 = {W.pos_of(4, at[k]) for k in ("ident", "off", "undec", "nonsub")} | {W.pos_of(4, 12)}
    honest2 = set(range(0, 32, 2))
    spoil = [1, 3, 31]                                                   # undecodable, off the curve, the identity: on good keys
    com = [4, 2, 4, 2, 5]
    pos_sets = [honest4 | bad4, honest2 | set(spoil), set(bad4) - {W.pos_of(4, 12)}, set(spoil), set(range(0, 129, 5))]
    msgs = [b"left out %d" % g for g in range(5)]
    entries = sign_positions(eng, W, com, pos_sets, msgs)
    for g in (1, 3):
        a, b, c = spoil
        entries[g][a] = b"\xff" * 32 + entries[g][a][32:]
        entries[g][b] = entries[g][b][:63] + bytes([entries[g][b][63] ^ 1])
        entries[g][c] = IDENT1
    s0 = eng.keyset_committee_aggregate_stats()
    res = eng.keyset_committee_aggregate_checked_batch(ks, com, entries, msgs, W.dst)
    s1 = eng.keyset_committee_aggregate_stats()
    want = yardstick(eng, ks, W, com, entries, msgs)
    assert res == want
    assert list(res[2]) == [0, 0, ST_SHORT, ST_SHORT, 0]
    kept0 = honest4 | (set() if checked else {W.pos_of(4, 12)})          # key 12 is a good key of the unchecked handle
    assert res[1][0] == row_of(kept0, 65) and res[1][1] == row_of(honest2, 32) and res[1][2] == bytes(9) and res[1][3] == bytes(4)
    assert delta(s1, s0) == {"optimistic_groups": 3, "fallback_groups": 0, "verified_signatures": 0, "short_groups": 2}


def wrong_case(eng, W):
    """group 0: one wrong signature among 40 of the 129-member committee; 1: every signature on another message; 2: P and -P
    alone; 3: two errors that cancel; 4, 5: honest neighbours (5 in the descending committee); 6: empty"""
    at = W.reg.at
    rnd = random.Random(9)
    com = [5, 3, 4, 2, 1, 3, 0]
    pos_sets = [set(rnd.sample(range(129), 40)), set(range(0, 33, 4)), {W.pos_of(4, at["p"]), W.pos_of(4, at["negp"])}, {2, 9, 17, 30}, set(range(31)), {0, 32, 5},
                set()]
    msgs = [b"one wrong %d" % g for g in range(7)]
    bad = (0, sorted(pos_sets[0])[17])
    entries = sign_positions(eng, W, com, pos_sets, msgs, sk=lambda g, p: W.reg.sk[W.coms[com[g]][p]] + 1 if (g, p) == bad else None)
    other = sign_positions(eng, W, com[1:2], pos_sets[1:2], [b"another message"])
    entries[1] = other[0]
    return com, pos_sets, msgs, entries, bad


def test_one_wrong_signature(eng, oracle, W, handles):
    ks = handles[False]
    com, pos_sets, msgs, entries, bad = wrong_case(eng, W)
    honest3 = dict(entries[3])
    G1 = oracle.g1_generator()
    d = random.Random(10).randrange(1, R)
    entries[3][2] = oracle.g1_add(honest3[2], oracle.g1_mul(G1, d))
    entries[3][17] = oracle.g1_add(honest3[17], oracle.g1_mul(G1, R - d))
    pk = b"".join(W.reg.keys[W.coms[2][p]] for p in (2, 17))
    assert eng.verify_batch(pk, [msgs[3]] * 2, entries[3][2] + entries[3][17], W.dst) == b"\x00"          # neither verifies on its own
    pn = sorted(pos_sets[2])
    assert eng.verify_batch(b"".join(W.reg.keys[W.coms[4][p]] for p in pn), [msgs[2]] * 2, b"".join(entries[2][p] for p in pn), W.dst) == b"\x03"
    s0 = eng.keyset_committee_aggregate_stats()
    res = eng.keyset_committee_aggregate_checked_batch(ks, com, entries, msgs, W.dst)
    s1 = eng.keyset_committee_aggregate_stats()
    y0 = eng.keyset_aggregate_stats()
    want = yardstick(eng, ks, W, com, entries, msgs)
    y1 = eng.keyset_aggregate_stats()
    assert res == want
    assert list(res[2]) == [0, ST_SHORT, ST_SHORT, 0, 0, 0, ST_SHORT]
    assert res[1][0] == row_of(pos_sets[0] - {bad[1]}, 129)              # the fallback drops exactly that entry
    assert res[1][1] == bytes(5) and res[1][2] == bytes(9) and res[0][64:192] == IDENT1 * 2
    assert res[1][3] == row_of(pos_sets[3], 32)                          # cancelling errors: both used
    assert res[0][192:256] == oracle.aggregate_sigs(b"".join(honest3[p] for p in sorted(honest3)), 4)
    assert res[1][5] == row_of(pos_sets[5], 33)
    assert delta(s1, s0) == delta(y1, y0) == {"optimistic_groups": 3, "fallback_groups": 3, "verified_signatures": 40 + 9 + 2, "short_groups": 3}
    bits = bits_of(eng.keyset_committee_fast_aggregate_verify_batch(ks, com, res[1], msgs, res[0], W.dst), len(com))
    assert [bool(b) for b in bits] == [s == 0 for s in res[2]]
    # a group's outcome depends on its own inputs only: the honest neighbours alone
    alone = eng.keyset_committee_aggregate_checked_batch(ks, com[4:6], entries[4:6], msgs[4:6], W.dst)
    assert alone == (res[0][256:384], res[1][4:6], res[2][4:6])


def test_launch_boundaries(eng, M, W, handles, monkeypatch):
    """contexts with 8, 16 and 64 lanes per launch: the cuts fall inside a group's entries (40 and 31 of them), between groups
    and inside a group's row words (5 for 129 members); the fallback's sub-call is cut likewise"""
    com, pos_sets, msgs, entries, bad = wrong_case(eng, W)
    want = eng.keyset_committee_aggregate_checked_batch(handles[False], com, entries, msgs, W.dst)
    assert want == yardstick(eng, handles[False], W, com, entries, msgs)
    many_com = [g % 4 for g in range(65)]
    many_pos = [{g % len(W.coms[c])} for g, c in enumerate(many_com)]
    many_msgs = [b"many %d" % g for g in range(65)]
    many = sign_positions(eng, W, many_com, many_pos, many_msgs)
    want64 = eng.keyset_committee_aggregate_checked_batch(handles[False], many_com[:64], many[:64], many_msgs[:64], W.dst)
    assert want64[2] == bytes(64)
    for chunk in ("8", "16", "64"):
        e = fresh_engine(M, monkeypatch, chunk)
        try:
            ks = W.keyset(M, e, False)
            assert e.keyset_committee_aggregate_stats() == ZERO
            assert e.keyset_committee_aggregate_checked_batch(ks, com, entries, msgs, W.dst) == want, chunk
            assert e.keyset_committee_aggregate_stats() == {"optimistic_groups": 3, "fallback_groups": 3, "verified_signatures": 51, "short_groups": 3}
            if chunk == "64":
                assert e.keyset_committee_aggregate_checked_batch(ks, many_com[:64], many[:64], many_msgs[:64], W.dst) == want64
                with pytest.raises(M.Bn254Error):
                    e.keyset_committee_aggregate_checked_batch(ks, many_com, many, many_msgs, W.dst)
                assert b"launch chunk" in e._lib.blsbn254_last_error(e._ctx)
            ks.close()
        finally:
            e.close()


def test_call_sequences_on_one_context(eng, oracle, M, W):
    """the new call between the full-width checked call, a committee verify and verify_batch, and again with other shapes: every
    result equals that of a context of its own (the shared buffers gs_sum, in_* and the committee workspace)"""
    com_a, pos_a, msgs_a, ent_a, _ = wrong_case(eng, W)                  # needs the fallback
    com_b, pos_b, msgs_b = honest_case(W)
    com_b, pos_b, msgs_b = com_b[:12], pos_b[:12], msgs_b[:12]
    ent_b = sign_positions(eng, W, com_b, pos_b, msgs_b)
    wide_b = [{W.coms[c][p]: s for p, s in es.items()} for c, es in zip(com_b, ent_b)]
    vb = synth.make_batch_gpu(eng, oracle, 200, W.dst, pool=16, invalid_every=7, spot=2)

    def verify_b(e, ks):
        out, rows, st = e.keyset_committee_aggregate_checked_batch(ks, com_b, ent_b, msgs_b, W.dst)
        return e.keyset_committee_fast_aggregate_verify_batch(ks, com_b, rows, msgs_b, out, W.dst)

    steps = [
        lambda e, ks: e.keyset_committee_aggregate_checked_batch(ks, com_a, ent_a, msgs_a, W.dst),
        lambda e, ks: e.keyset_aggregate_checked_batch(ks, wide_b, msgs_b, W.dst),
        verify_b,
        lambda e, ks: e.verify_batch(vb[0], vb[1], vb[2], W.dst),
        lambda e, ks: e.keyset_committee_aggregate_checked_batch(ks, com_b, ent_b, msgs_b, W.dst),
        lambda e, ks: e.keyset_committee_aggregate_checked_batch(ks, com_a, ent_a, msgs_a, W.dst),
    ]

    def run(which):
        e = M.Engine(0)
        try:
            ks = W.keyset(M, e, False)
            try:
                return [steps[j](e, ks) for j in which]
            finally:
                ks.close()
        finally:
            e.close()

    fresh = [run([j])[0] for j in range(len(steps))]
    assert fresh[3] == synth.bitmap_of(vb[3]) and fresh[0][2] == bytes([0, ST_SHORT, ST_SHORT, 0, 0, 0, ST_SHORT])
    got = run(range(len(steps)))
    for j, (a, b) in enumerate(zip(got, fresh)):
        assert a == b, "step %d differs from the same call on a context of its own" % j


def test_table_replacement(eng, M, W):
    """after set_committees replaces the table the same (com, positions) name other keys, and the call follows"""
    table_b = [W.coms[3][::-1], W.coms[5], W.coms[1]]
    com = [0, 1, 2, 0]
    pos_sets = [{0, 1, 32}, set(range(0, 129, 3)), {30, 7}, set(range(33))]
    msgs = [b"table %d" % g for g in range(4)]
    ks = W.keyset(M, eng, False, table=[W.coms[3], W.coms[5], W.coms[1]])
    try:
        ent_a = sign_positions(eng, W, com, pos_sets, msgs, coms=[W.coms[3], W.coms[5], W.coms[1]])
        res_a = eng.keyset_committee_aggregate_checked_batch(ks, com, ent_a, msgs, W.dst)
        assert res_a == yardstick(eng, ks, W, com, ent_a, msgs, coms=[W.coms[3], W.coms[5], W.coms[1]]) and res_a[2] == bytes(4)
        ks.set_committees(table_b)
        ent_b = sign_positions(eng, W, com, pos_sets, msgs, coms=table_b)
        res_b = eng.keyset_committee_aggregate_checked_batch(ks, com, ent_b, msgs, W.dst)
        assert res_b == yardstick(eng, ks, W, com, ent_b, msgs, coms=table_b) and res_b[2] == bytes(4)
        assert res_b[0][:64] != res_a[0][:64] and res_b[0][192:] == res_a[0][192:]      # positions 0, 1, 32 name other keys now; the full committee is the same set
        # the old table's signatures under the new table: members 0 and 32 of the reversed list did not sign these
        stale = eng.keyset_committee_aggregate_checked_batch(ks, com[:1], ent_a[:1], msgs[:1], W.dst)
        assert stale == yardstick(eng, ks, W, com[:1], ent_a[:1], msgs[:1], coms=table_b) and stale[2] == bytes([ST_SHORT])
    finally:
        ks.close()


def test_argument_errors(eng, M, W):
    lib, ctx = eng._lib, eng._ctx
    u8, u32, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    dst = b"TEST"
    coms = [list(range(13)), list(range(8, 24))]                         # rows of 2 bytes
    com_l, pos_sets, msgs = [0, 1], [{0, 1, 12}, {5}], [b"a", b"bc"]
    sets = [{coms[c][p] for p in ps} for c, ps in zip(com_l, pos_sets)]
    by_key = sign_sets(eng, W.reg, sets, msgs, dst)
    sg = np.frombuffer(b"".join(by_key[g][coms[c][p]] for g, c in enumerate(com_l) for p in sorted(pos_sets[g])), dtype=np.uint8)
    data = np.frombuffer(b"abc", dtype=np.uint8)
    out = np.zeros(128, dtype=np.uint8); sel = np.zeros(4, dtype=np.uint8); st = np.zeros(2, dtype=np.uint8)
    P = lambda a: a.ctypes.data_as(u8)
    keep = []

    def arr(v, t):
        a = np.array(v, dtype=t); keep.append(a)
        return a.ctypes.data_as(u32 if t == np.uint32 else u64)

    ks = M.KeySet(eng, W.reg.pks, W.n)
    bare = M.KeySet(eng, W.reg.pks, W.n)                                # a handle without a committee table
    ks.set_committees(coms)
    h = ks._h

    def call(c=ctx, k=h, cm=(0, 1), p=(0, 1, 12, 5), s=P(sg), so=(0, 3, 4), m=P(data), mo=(0, 1, 3), ro=(0, 2, 4), g=2, d=dst, dl=4, o=P(out), r=P(sel), t=P(st)):
        cm = arr(cm, np.uint32) if cm is not None else None
        p = arr(p, np.uint32) if p is not None else None
        so, mo, ro = (arr(x, np.uint64) if x is not None else None for x in (so, mo, ro))
        return lib.blsbn254_keyset_committee_aggregate_checked_batch(c, k, cm, p, s, so, m, mo, ro, ctypes.c_size_t(g), d, ctypes.c_size_t(dl), o, r, t)

    def untouched():
        return out.tobytes() == b"\x5a" * 128 and sel.tobytes() == b"\x5a" * 4 and st.tobytes() == b"\x5a" * 2

    def err():
        return lib.blsbn254_last_error(ctx)

    try:
        out[:] = 0x5a; sel[:] = 0x5a; st[:] = 0x5a
        stats0 = eng.keyset_committee_aggregate_stats()
        eng.profile_enable(True); eng.profile_reset()                   # every kernel launch of this context is recorded from here on
        for name in ("c", "k", "cm", "p", "s", "so", "m", "mo", "ro", "d", "o", "r", "t"):
            assert call(**{name: None}) == E_ARG and untouched(), name
        e2 = M.Engine(0)                                                # a key set that belongs to another context
        try:
            assert call(c=e2._ctx) == E_ARG and untouched()
        finally:
            e2.close()
        assert call(k=bare._h) == E_ARG and b"no committees" in err()
        assert call(cm=(0, 2)) == E_ARG and b"group 1 names committee 2 of 2" in err()
        assert call(p=(0, 1, 13, 5)) == E_ARG and b"entry 2 names no member" in err()
        assert call(p=(0, 1, 12, 16)) == E_ARG and b"entry 3 names no member" in err()
        assert call(p=(0, 1, 1, 5)) == E_ARG and b"group 0" in err() and b"strictly increase" in err()
        assert call(p=(0, 12, 1, 5)) == E_ARG and b"group 0" in err() and b"strictly increase" in err()
        assert call(so=(0, 3, 2)) == E_ARG and b"offsets decrease" in err()
        assert call(mo=(0, 2, 1)) == E_ARG and b"offsets decrease" in err()
        assert call(ro=(0, 2, 1)) == E_ARG and b"offsets decrease" in err()
        assert call(ro=(0, 2, 3)) == E_ARG and b"group 1: the row must be 2 bytes" in err()
        assert call(ro=(0, 3, 5)) == E_ARG and b"group 0: the row must be 2 bytes" in err()
        assert call(so=(0, 3, (1 << 23) + 1)) == E_ARG and b"2^23" in err()
        assert call(g=(1 << 22) + 1) == E_ARG and b"launch chunk" in err()
        assert lib.blsbn254_keyset_committee_aggregate_stats(ctx, None) == E_ARG
        assert lib.blsbn254_keyset_committee_aggregate_stats(None, (ctypes.c_uint64 * 4)()) == E_ARG
        assert call(g=0) == 0 and call(g=0, cm=None, p=None, s=None, so=None, m=None, mo=None, ro=None, o=None, r=None, t=None) == 0
        launched = eng.profile_read()
        eng.profile_enable(False); eng.profile_reset()
        assert untouched() and launched == {} and eng.keyset_committee_aggregate_stats() == stats0       # nothing was enqueued or counted
        assert call() == 0 and st.tobytes() == bytes(2)                 # after the errors, the context still serves
        assert sel.tobytes() == row_of(pos_sets[0], 13) + row_of(pos_sets[1], 16) and out.tobytes()[64:] == by_key[1][coms[1][5]]
        # offsets that do not start at 0: one leading entry, message bytes and row offset that are not looked at
        first = out.tobytes()
        out[:] = 0x5a; sel[:] = 0x5a
        lead_s = np.concatenate([np.zeros(64, dtype=np.uint8), sg])
        lead_m = np.frombuffer(b"??abc", dtype=np.uint8)
        assert call(p=(99, 0, 1, 12, 5), s=P(lead_s), so=(1, 4, 5), m=P(lead_m), mo=(2, 3, 5), ro=(1000, 1002, 1004)) == 0 and st.tobytes() == bytes(2)
        assert sel.tobytes() == row_of(pos_sets[0], 13) + row_of(pos_sets[1], 16) and out.tobytes() == first
        with pytest.raises(ValueError):
            eng.keyset_committee_aggregate_checked_batch(ks, [0], [[(1, by_key[0][1]), (1, by_key[0][1])]], [b"a"], dst)
        with pytest.raises(ValueError):
            eng.keyset_committee_aggregate_checked_batch(ks, [0], [{0: by_key[0][0]}], [], dst)
        assert eng.keyset_committee_aggregate_checked_batch(ks, [], [], [], dst) == (b"", [], b"")
    finally:
        eng.profile_enable(False)
        ks.close(); bare.close()
