"""GPU tests (MI355X) of the committees over a registered key set (blsbn254_keyset_set_committees and the three calls over ragged
groups, blsbn254_keyset_committee_*).  The yardstick throughout is the EXISTING full-width call on the rows scattered over the
registry, byte for byte and bit for bit; the sums at 70 keys are also checked against the oracle's sums of the listed keys."""
import ctypes
import random

import numpy as np
import pytest

import blsbn254_loader
from tests import synth
from tests.gpu_support import eng, fresh_engine, M
from tests.helpers import b32, bits_of, IDENT1, IDENT2, row_of
from tests.keyset_support import Committee, committee_model_plan, sign_rows

pytestmark = pytest.mark.gpu
E_ARG = -1
_M = blsbn254_loader.load()
_M.KeySet.set_committees, _M.Engine.keyset_committee_sum_batch          # the feature is there, or this module does not import


def scatter(members, positions):
    return {members[j] for j in positions}


class World:
    """700 keys (not a multiple of 32) with an undecodable key, an off-curve key, an identity key, a key outside the r-torsion
    and, on the checked handle, a key whose proof fails (12).  Committees of 1, 31, 32, 33, 64, 65, 257 and 545 members: 1 and 2
    overlap, 3 lists its members in descending order, 4 contains the off-curve key 5 (and 12), 5 the identity key 3, 7 is a
    random sample that contains the undecodable key.  Groups: per committee the empty row, the full row (the complement with
    nothing to subtract), exactly half, half + 1, and for a committee with a bad key one row that selects it and one that leaves
    only the bad keys out (flipped, stays valid); committee 2 gets 70 random rows more, which crosses an item.  The caller's
    order interleaves the committees."""

    def __init__(self, eng, M):
        self.dst = M.DEFAULT_DST
        self.n = n = 700
        rnd = random.Random(2026)
        self.reg = reg = Committee(eng, n, 61)
        at = reg.at
        first = [reg.sk[i] if reg.sk[i] else 1000 + i for i in range(n)]
        p = eng.pop_prove_batch(b"".join(b32(s) for s in first), n)
        # proofs fail for key 12 (replaced) and for the keys nobody holds a secret for: the identity key and the one outside the r-torsion
        self.proof_fails = {12, at["ident"], at["nonsub"]}
        self.proofs = p[:64 * 12] + IDENT1 + p[64 * 13:]
        rest = [i for i in range(n) if i != at["undec"]]
        self.coms = [[20], list(range(100, 131)), list(range(120, 152)), list(range(232, 199, -1)), list(range(4, 68)),
                     [at["ident"]] + list(range(300, 364)), list(range(400, 657)), sorted(rnd.sample(rest, 544) + [at["undec"]])]
        assert [len(c) for c in self.coms] == [1, 31, 32, 33, 64, 65, 257, 545]
        assert set(self.coms[1]) & set(self.coms[2]) and at["off"] in self.coms[4] and 12 in self.coms[4]
        groups = []
        for c, mem in enumerate(self.coms):
            s = len(mem)
            full = set(range(s))
            badpos = {j for j, i in enumerate(mem) if i in reg.bad or i == 12}
            nosign = {j for j, i in enumerate(mem) if i in reg.unsignable or i == 12}
            clean = sorted(full - nosign)
            groups += [(c, set()), (c, full), (c, set(rnd.sample(clean, min(len(clean), s // 2)))), (c, set(rnd.sample(clean, min(len(clean), s // 2 + 1))))]
            if badpos:
                groups += [(c, {min(badpos), clean[0]}), (c, full - badpos)]
        groups += [(2, {j for j in range(32) if rnd.random() < (0.3, 0.7)[g & 1]}) for g in range(70)]
        rnd.shuffle(groups)
        self.groups = groups
        self.com = [c for c, _ in groups]
        self.rows = [row_of(r, len(self.coms[c])) for c, r in groups]
        self.sets = [scatter(self.coms[c], r) for c, r in groups]      # the keys a row names, as registry indices
        self.wide = [row_of(s, n) for s in self.sets]
        self.G = G = len(groups)
        self.msgs = [b"committee %d" % g for g in range(G)]
        sigs = sign_rows(eng, reg, self.sets, self.msgs, self.dst)
        big = [g for g in range(G) if len(self.sets[g]) > 8 and not (self.sets[g] & (reg.unsignable | {12}))]
        self.tampered, self.ident_sig = big[0], big[1]
        self.msgs[self.tampered] += b"!"
        sigs[64 * self.ident_sig:64 * self.ident_sig + 64] = IDENT1
        self.sigs = bytes(sigs)
        self.flips = sum(1 for c, r in groups if 2 * len(r) > len(self.coms[c]))

    def keyset(self, M, e, checked):
        ks = M.KeySet(e, self.reg.pks, self.n, proofs=self.proofs if checked else None)
        ks.set_committees(self.coms)
        return ks


@pytest.fixture(scope="module")
def W(eng, M):
    return World(eng, M)


@pytest.fixture(scope="module")
def handles(eng, M, W):
    hs = {False: W.keyset(M, eng, False), True: W.keyset(M, eng, True)}
    yield hs
    for ks in hs.values():
        ks.close()


def test_shape_of_the_case(W):
    assert W.G >= 100 and W.com.count(2) >= 74 and W.flips >= 12
    runs = sum(1 for a, b in zip(W.com, W.com[1:]) if a != b)
    assert runs > W.G // 3                                              # the caller's order interleaves the committees
    assert any(W.reg.at["off"] in s and 2 * len(r) <= 64 for s, (c, r) in zip(W.sets, W.groups) if c == 4)
    assert any(c == 4 and 2 * len(r) > 64 and not (s & (W.reg.bad | {12})) for s, (c, r) in zip(W.sets, W.groups))


@pytest.mark.parametrize("checked", [False, True])
def test_sums_equal_the_full_width_call(eng, W, handles, checked):
    ks = handles[checked]
    assert ks.committee_count() == 8 and ks.checked() is checked
    s0, f0 = eng.keyset_committee_stats(), eng.keyset_stats()
    out, status = eng.keyset_committee_sum_batch(ks, W.com, W.rows)
    s1, f1 = eng.keyset_committee_stats(), eng.keyset_stats()
    want_out, want_status = eng.keyset_sum_batch(ks, W.wide)
    assert status == want_status and out == want_out
    bad = W.reg.bad | (W.proof_fails if checked else set())
    assert list(status) == [0 if s & bad else 1 for s in W.sets] and 0 < sum(status) < W.G
    assert all(out[128 * g:128 * g + 128] == IDENT2 for g in range(W.G) if not status[g] or not W.sets[g])
    assert f1 == f0                                                     # blsbn254_keyset_stats does not count these calls
    assert s1["groups"] - s0["groups"] == W.G and s1["complement_groups"] - s0["complement_groups"] == W.flips
    assert s1["launches"] - s0["launches"] == 1 and s1["tables"] == s0["tables"]


@pytest.mark.parametrize("checked", [False, True])
def test_verify_equals_the_full_width_call(eng, W, handles, checked):
    ks = handles[checked]
    got = eng.keyset_committee_fast_aggregate_verify_batch(ks, W.com, W.rows, W.msgs, W.sigs, W.dst)
    want = eng.keyset_fast_aggregate_verify_batch(ks, W.wide, W.msgs, W.sigs, W.dst)
    assert got == want
    bits = bits_of(got, W.G)
    assert not bits[W.tampered] and not bits[W.ident_sig]
    excluded = W.reg.unsignable | W.proof_fails                         # (key 12 is a good key of the unchecked handle; left out all the same)
    good = [g for g in range(W.G) if W.sets[g] and not (W.sets[g] & excluded) and g not in (W.tampered, W.ident_sig)
            and W.reg.group_sk(W.sets[g]) == sum(W.reg.sk[i] for i in W.sets[g]) % synth.R]
    assert len(good) > W.G // 3 and all(bits[g] for g in good)
    # a flipped row of committee 4 that leaves its bad keys unselected verifies; one that selects the off-curve key does not
    for g, (c, r) in enumerate(W.groups):
        if c == 4 and W.reg.at["off"] in W.sets[g]:
            assert not bits[g]


@pytest.mark.parametrize("nc", [1, 4])
def test_weights_equal_the_full_width_call(eng, W, handles, nc):
    rnd = random.Random(40 + nc)
    pool = [0, 1, (1 << 32) - 1, 1 << 32, ((1 << 64) - 1) // W.n]
    cols = [[rnd.choice(pool) for _ in range(W.n)] for _ in range(nc)]
    for checked, ks in handles.items():
        ks.set_weights(cols)
        got = eng.keyset_committee_weight_batch(ks, W.com, W.rows)
        want = eng.keyset_weight_batch(ks, W.wide)
        assert got.shape == (W.G, nc) and got.dtype == np.uint64 and got.tolist() == want.tolist()
        valid = bits_of(ks.valid_bitmap(), W.n)
        assert not valid[12] or not checked
        assert got.tolist() == [[sum(col[i] for i in s if valid[i]) for col in cols] for s in W.sets]
        tot = ks.committee_total_weight()
        assert tot.tolist() == eng.keyset_weight_batch(ks, [row_of(c, W.n) for c in W.coms]).tolist()
        assert eng.keyset_committee_weight_batch(ks, [], []).shape == (0, nc)


def test_sums_at_70_keys_against_the_oracle(eng, oracle, M):
    n = 70
    rnd = random.Random(7)
    reg = Committee(eng, n, 62)
    coms = [[7], list(range(69, 36, -1)), list(range(0, 40)), [1, 2, 4, 6, 8, 3], list(range(30, 66))]
    groups = []
    for c, mem in enumerate(coms):
        s = len(mem)
        groups += [(c, set()), (c, set(range(s))), (c, set(rnd.sample(range(s), s // 2))), (c, set(rnd.sample(range(s), s // 2 + 1)))]
        groups += [(c, {j for j in range(s) if mem[j] not in reg.bad})]
    rnd.shuffle(groups)
    ks = M.KeySet(eng, reg.pks, n)
    try:
        ks.set_committees(coms)
        out, status = eng.keyset_committee_sum_batch(ks, [c for c, _ in groups], [row_of(r, len(coms[c])) for c, r in groups])
        wide = eng.keyset_sum_batch(ks, [row_of(scatter(coms[c], r), n) for c, r in groups])
    finally:
        ks.close()
    assert (out, status) == wide
    for g, (c, r) in enumerate(groups):
        keys = scatter(coms[c], r)
        assert status[g] == (0 if keys & reg.bad else 1)
        want = oracle.aggregate_pks(reg.gather(keys), len(keys)) if status[g] else IDENT2
        assert out[128 * g:128 * g + 128] == want, (g, c)
    assert 0 < sum(status) < len(groups)


def test_many_small_committees(eng, M, W):
    """the shape of a slot: 2048 overlapping committees of 32 members over the 700 keys, 2 groups each in an order that separates
    them, so that every item is one word of one committee across two lanes"""
    rnd = random.Random(99)
    n_com = 2048
    coms = [rnd.sample(range(W.n), 32) for _ in range(n_com)]
    com = list(range(n_com)) + list(range(n_com - 1, -1, -1))
    pos = [{j for j in range(32) if rnd.random() < (0.4, 0.7)[g & 1]} for g in range(len(com))]
    ks = M.KeySet(eng, W.reg.pks, W.n)
    try:
        ks.set_committees(coms)
        assert ks.committee_count() == n_com
        s0 = eng.keyset_committee_stats()
        got = eng.keyset_committee_sum_batch(ks, com, [row_of(r, 32) for r in pos])
        s1 = eng.keyset_committee_stats()
        want = eng.keyset_sum_batch(ks, [row_of(scatter(coms[c], r), W.n) for c, r in zip(com, pos)])
    finally:
        ks.close()
    assert got == want and 0 < sum(got[1]) < len(com)
    assert s1["groups"] - s0["groups"] == len(com) and s1["launches"] - s0["launches"] == 1
    assert s1["complement_groups"] - s0["complement_groups"] == sum(1 for r in pos if len(r) > 16)


def test_launch_boundaries(eng, M, W, handles, monkeypatch):
    """the same calls on contexts with 512 and with 64 lanes per launch.  64: 60 groups (such a context takes no more than 64 in
    one call), the 545-member rows of 18 partials each among them; 512: the whole case three times over"""
    rest = [g for g in range(W.G) if W.com[g] != 2]
    pick = sorted(rest + [g for g in range(W.G) if W.com[g] == 2][:60 - len(rest)])
    assert len(pick) == 60 and sum(1 for g in pick if W.com[g] == 7) == 6
    cols = [[i + 1 for i in range(W.n)], [1 << 33] * W.n]
    ks0 = handles[False]
    ks0.set_weights(cols)
    for chunk, groups, min_launches in (("512", list(range(W.G)) * 3, 2), ("64", pick, 4)):
        com, rows = [W.com[g] for g in groups], [W.rows[g] for g in groups]
        msgs, sigs = [W.msgs[g] for g in groups], b"".join(W.sigs[64 * g:64 * g + 64] for g in groups)
        want = (eng.keyset_committee_sum_batch(ks0, com, rows), eng.keyset_committee_fast_aggregate_verify_batch(ks0, com, rows, msgs, sigs, W.dst),
                eng.keyset_committee_weight_batch(ks0, com, rows).tolist())
        assert want[0] == eng.keyset_sum_batch(ks0, [W.wide[g] for g in groups])
        launches = len(committee_model_plan(W.coms, com, int(chunk))[1])
        assert launches >= min_launches and len(groups) <= int(chunk)
        e = fresh_engine(M, monkeypatch, chunk)
        try:
            ks = W.keyset(M, e, False)
            ks.set_weights(cols)
            assert e.keyset_committee_stats() == {"groups": 0, "complement_groups": 0, "launches": 0, "tables": 1}
            got = (e.keyset_committee_sum_batch(ks, com, rows), e.keyset_committee_fast_aggregate_verify_batch(ks, com, rows, msgs, sigs, W.dst),
                   e.keyset_committee_weight_batch(ks, com, rows).tolist())
            assert got == want, chunk
            st = e.keyset_committee_stats()
            assert st["launches"] == 2 * launches and st["groups"] == 3 * len(groups)
            if chunk == "64":
                with pytest.raises(M.Bn254Error):
                    e.keyset_committee_sum_batch(ks, W.com[:65], W.rows[:65])
            ks.close()
        finally:
            e.close()


def test_call_sequences_on_one_context(M, W):
    """set_committees twice with different tables and a full-width call in between: each result equals the same call on a
    fresh context"""
    table_b = [W.coms[7], W.coms[3][::-1], W.coms[2]]
    remap = {7: 0, 3: 1, 2: 2}
    pick_b = [g for g in range(W.G) if W.com[g] in (7, 2)][:40]

    def com_a(e, ks):
        ks.set_committees(W.coms)
        return e.keyset_committee_sum_batch(ks, W.com, W.rows), e.keyset_committee_fast_aggregate_verify_batch(ks, W.com, W.rows, W.msgs, W.sigs, W.dst)

    def wide(e, ks):
        return e.keyset_fast_aggregate_verify_batch(ks, W.wide, W.msgs, W.sigs, W.dst), e.keyset_sum_batch(ks, W.wide[:9])

    def com_b(e, ks):
        ks.set_committees(table_b)
        assert ks.committee_count() == 3
        return e.keyset_committee_sum_batch(ks, [remap[W.com[g]] for g in pick_b], [W.rows[g] for g in pick_b])

    def run(seq):
        e = M.Engine(0)
        try:
            ks = M.KeySet(e, W.reg.pks, W.n)
            out = [f(e, ks) for f in seq]
            ks.close()
            return out
        finally:
            e.close()

    alone = {f: run([f])[0] for f in (com_a, wide, com_b)}
    assert alone[com_a][1] == alone[wide][0] and alone[com_a][0][0][:128 * 9] == alone[wide][1][0]
    for seq in ([com_a, wide, com_b, wide, com_a], [com_b, com_a, wide, com_b]):
        assert run(seq) == [alone[f] for f in seq]


def test_argument_errors(eng, M):
    lib, ctx = eng._lib, eng._ctx
    n = 40
    reg = Committee(eng, n, 63, special=False)
    coms = [list(range(13)), list(range(8, 24))]                        # rows of 2 bytes: 3 padding bits, none
    u8, u32, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    com = np.array([0, 1, 0], dtype=np.uint32)
    sel = np.frombuffer(row_of([0, 12], 13) + row_of([15], 16) + row_of(range(13), 13), dtype=np.uint8).copy()
    so = np.array([0, 2, 4, 6], dtype=np.uint64)
    out = np.zeros(3 * 128, dtype=np.uint8); st = np.zeros(3, dtype=np.uint8); bm = np.zeros(1, dtype=np.uint8)
    wout = np.zeros(3, dtype=np.uint64)
    msgs = np.frombuffer(b"abcdef", dtype=np.uint8); off = np.array([0, 1, 3, 6], dtype=np.uint64)
    sigs = np.frombuffer(bytes(sign_rows(eng, reg, [{0, 12}, {23}, set(range(13))], [b"a", b"bc", b"def"], b"TEST")), dtype=np.uint8)
    ks = M.KeySet(eng, reg.pks, n)
    h = ks._h

    def sums(c=ctx, k=h, cm=com, s=sel, o=so, g=3):
        return lib.blsbn254_keyset_committee_sum_batch(c, k, cm.ctypes.data_as(u32), s.ctypes.data_as(u8), o.ctypes.data_as(u64), ctypes.c_size_t(g),
                                                       out.ctypes.data_as(u8), st.ctypes.data_as(u8))

    def verify(c=ctx, k=h, cm=com, s=sel, o=so, g=3):
        return lib.blsbn254_keyset_committee_fast_aggregate_verify_batch(c, k, cm.ctypes.data_as(u32), s.ctypes.data_as(u8), o.ctypes.data_as(u64),
                                                                         msgs.ctypes.data_as(u8), off.ctypes.data_as(u64), sigs.ctypes.data_as(u8), ctypes.c_size_t(g),
                                                                         b"TEST", ctypes.c_size_t(4), bm.ctypes.data_as(u8))

    def weigh(c=ctx, k=h, cm=com, s=sel, o=so, g=3):
        return lib.blsbn254_keyset_committee_weight_batch(c, k, cm.ctypes.data_as(u32), s.ctypes.data_as(u8), o.ctypes.data_as(u64), ctypes.c_size_t(g),
                                                          wout.ctypes.data_as(u64))

    def setc(lists, c=ctx, k=h):
        flat = np.array([i for l in lists for i in l] or [0], dtype=np.uint32)
        o = np.cumsum([0] + [len(l) for l in lists]).astype(np.uint64)
        return lib.blsbn254_keyset_set_committees(c, k, flat.ctypes.data_as(u32), o.ctypes.data_as(u64), ctypes.c_size_t(len(lists)))

    try:
        prof0 = eng.keyset_committee_stats()
        # no table on the handle
        assert ks.committee_count() == 0
        for f in (sums, verify):
            assert f() == E_ARG and b"no committees" in lib.blsbn254_last_error(ctx)
        ks2 = M.KeySet(eng, reg.pks, n)                                 # ... and weight_batch, on a handle that has its stake table
        try:
            ks2.set_weights([[1] * n])
            assert weigh(k=ks2._h) == E_ARG and b"no committees" in lib.blsbn254_last_error(ctx)
        finally:
            ks2.close()
        # tables that are refused leave none / the old one
        assert setc([[0, 1], [4, 5, 4]]) == E_ARG and b"committee 1" in lib.blsbn254_last_error(ctx) and ks.committee_count() == 0
        assert setc(coms) == 0 and ks.committee_count() == 2
        for lists in ([[0, 1], [4, 5, 4]], [[0], [n]], [[0], []], []):
            assert setc(lists) == E_ARG and ks.committee_count() == 2, lists
        bad_off = np.array([0, 3, 2, 4], dtype=np.uint64)
        assert lib.blsbn254_keyset_set_committees(ctx, h, com.ctypes.data_as(u32), bad_off.ctypes.data_as(u64), ctypes.c_size_t(3)) == E_ARG
        assert b"committee 1" in lib.blsbn254_last_error(ctx) and ks.committee_count() == 2
        with pytest.raises(M.Bn254Error):
            ks.set_committees([[1, 1]])
        # weight without stake
        assert weigh() == E_ARG and b"no weights" in lib.blsbn254_last_error(ctx)
        ks.set_weights([list(range(1, n + 1))])
        good = (sums(), bytes(out), bytes(st), verify(), int(bm[0]), weigh(), wout.tolist())
        assert good[0] == 0 and good[3] == 0 and good[5] == 0 and good[2] == b"\x01\x01\x01" and good[4] == 7
        assert good[6] == [1 + 13, 24, 91]
        served = eng.keyset_committee_stats()
        assert served["groups"] - prof0["groups"] == 9 and served["tables"] - prof0["tables"] == 1
        k3 = M.KeySet(eng, reg.pks, n)                                  # a handle without a table, registered before the recording starts
        eng.profile_enable(True); eng.profile_reset()                   # every kernel launch of this context is recorded from here on
        for f in (sums, verify, weigh):
            # a wrong row length, a padding bit, com[g] = n_com, a key set of another context
            assert f(o=np.array([0, 2, 3, 5], dtype=np.uint64)) == E_ARG and b"group 1" in lib.blsbn254_last_error(ctx)
            padded = sel.copy(); padded[5] |= 0x20
            assert f(s=padded) == E_ARG and b"group 2" in lib.blsbn254_last_error(ctx)
            assert f(cm=np.array([0, 2, 0], dtype=np.uint32)) == E_ARG and b"group 1" in lib.blsbn254_last_error(ctx)
            e2 = M.Engine(0)
            try:
                e2.profile_enable(True)
                assert f(c=e2._ctx) == E_ARG and e2.profile_read() == {}
                assert e2.keyset_committee_stats() == {"groups": 0, "complement_groups": 0, "launches": 0, "tables": 0}
            finally:
                e2.close()
            assert f(g=0) == 0
        assert sums(k=k3._h) == E_ARG and verify(k=k3._h) == E_ARG and b"no committees" in lib.blsbn254_last_error(ctx)
        launched = eng.profile_read()
        eng.profile_enable(False); eng.profile_reset()
        k3.close()
        assert launched == {} and eng.keyset_committee_stats() == served    # the refused calls launched nothing
        assert (sums(), bytes(out), bytes(st), verify(), int(bm[0]), weigh(), wout.tolist()) == good       # the context still serves
        assert lib.blsbn254_keyset_committee_stats(ctx, None) == E_ARG and lib.blsbn254_keyset_committee_stats(None, (ctypes.c_uint64 * 4)()) == E_ARG
        with pytest.raises(ValueError):
            eng.keyset_committee_sum_batch(ks, [0], [])
    finally:
        ks.close()
