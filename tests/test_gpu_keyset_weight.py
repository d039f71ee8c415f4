"""GPU tests (MI355X) of the stake weights on a registered key set (blsbn254_keyset_set_weights / _weight_batch) and of
FastAggregateVerify with a quorum (blsbn254_keyset_quorum_verify_batch).  Expected weights are Python sums over the selected
keys that have the validity bit; expected verification bits are the Python quorum rule on those ANDed with the bits of
blsbn254_keyset_fast_aggregate_verify_batch on all groups."""
import ctypes
import random

import numpy as np
import pytest

from tests import synth
from tests.gpu_support import eng, fresh_engine, M
from tests.helpers import b32, bits_of, IDENT1, row_of
from tests.keyset_support import Committee, edge_rows, sign_rows

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
E_ARG = -1


def table(rnd, n, nc):
    """columns whose sums fit 64 bits, with entries that carry across the 32-bit halves of the reduction"""
    pool = [0, 1, (1 << 32) - 1, 1 << 32, M64 // n]
    return [[rnd.choice(pool) for _ in range(n)] for _ in range(nc)]


def expect(cols, rows, valid):
    return [[sum(col[i] for i in r if valid[i]) for col in cols] for r in rows]


@pytest.mark.parametrize("n", [1, 33, 70, 513, 2081])
def test_weights_against_python_sums(eng, M, n):
    rnd = random.Random(500 + n)
    com = Committee(eng, n, 30 + n, special=n < 2081)
    assert ((n + 31) // 32, (n + 7) // 8) == {1: (1, 1), 33: (2, 5), 70: (3, 9), 513: (17, 65), 2081: (66, 261)}[n]
    proofs = None
    if com.at:                                                          # ... and one key whose proof of possession fails
        first = [synth.sk_of(1000 * (30 + n) + k) for k in range(n)]
        p = eng.pop_prove_batch(b"".join(b32(com.sk[i] if com.sk[i] else first[i]) for i in range(n)), n)
        proofs = p[:64 * 12] + IDENT1 + p[64 * 13:]
    rows, _ = edge_rows(com, rnd)
    nine = [{i for i in range(n) if rnd.random() < 0.5} for _ in range(9)]      # two workgroups of four waves and one group over
    ks = M.KeySet(eng, com.pks, n, proofs=proofs)
    try:
        valid = bits_of(ks.valid_bitmap(), n)
        if com.at:
            at = com.at
            invalid = {at["ident"], at["nonsub"], at["off"], at["undec"], 12}
            assert {i for i in range(n) if not valid[i]} == invalid
            rows += [invalid, set(range(n)) - invalid]
        t0 = eng.keyset_weight_stats()
        for nc in (1, 3, 8):
            cols = table(rnd, n, nc)
            if com.at:
                for i in invalid:                                       # plain arithmetic would show these
                    cols[0][i] = M64 // n
            ks.set_weights(cols)
            assert ks.total_weight() == expect(cols, [set(range(n))], valid)[0]
            for rs in (rows, nine):
                got = eng.keyset_weight_batch(ks, [row_of(r, n) for r in rs])
                assert got.shape == (len(rs), nc) and got.dtype == np.uint64
                assert got.tolist() == expect(cols, rs, valid), (n, nc)
            if com.at:
                assert eng.keyset_weight_batch(ks, [row_of(invalid, n)]).tolist() == [[0] * nc]
        t1 = eng.keyset_weight_stats()
        assert t1["tables"] - t0["tables"] == 3 and t1["launches"] - t0["launches"] == (9 if com.at else 6)
        assert t1["groups"] - t0["groups"] == 3 * (len(rows) + 9) + (3 if com.at else 0) and t1["below_quorum"] == t0["below_quorum"]
        # the last table (eight columns) replaced by one column: nothing of the old one is left
        ks.set_weights([[3] * n])
        assert ks.total_weight() == [3 * sum(valid)]
        assert eng.keyset_weight_batch(ks, [row_of(range(n), n), row_of([], n)]).tolist() == [[3 * sum(valid)], [0]]
        assert eng.keyset_weight_batch(ks, []).shape == (0, 1)
    finally:
        ks.close()


def test_rows_of_the_checked_aggregation_are_rows_of_the_weights(eng, M):
    dst = M.DEFAULT_DST
    n = 70
    com = Committee(eng, n, 41)
    signers = [i for i in range(n) if com.sk[i]][:9] + [com.at["nonsub"]]
    msgs = [b"weigh the collected row"]
    ss = eng.sign_batch(b"".join(b32(com.sk[i] or 5) for i in signers), msgs * len(signers), dst)
    ks = M.KeySet(eng, com.pks, n)
    try:
        ks.set_weights([list(range(1, n + 1))])
        _, out_sel, status = eng.keyset_aggregate_checked_batch(ks, [[(i, ss[64 * j:64 * j + 64]) for j, i in enumerate(signers)]], msgs, dst)
        assert status == b"\x00" and out_sel == row_of(signers[:9], n)
        assert eng.keyset_weight_batch(ks, out_sel).tolist() == [[sum(i + 1 for i in signers[:9])]]
    finally:
        ks.close()


def test_launch_boundaries_of_the_weights(eng, M, monkeypatch):
    n, G = 70, 41
    rnd = random.Random(9)
    com = Committee(eng, n, 42)
    rows = [row_of({i for i in range(n) if rnd.random() < 0.6}, n) for _ in range(G)]
    cols = table(rnd, n, 3)
    res = []
    for chunk, launches in ((None, 1), ("512", 6), ("64", 41)):         # 512 lanes: launches of 8 groups; 64: a group each
        e = fresh_engine(M, monkeypatch, chunk)
        try:
            ks = M.KeySet(e, com.pks, n)
            ks.set_weights(cols)
            res.append(e.keyset_weight_batch(ks, rows).tolist())
            assert e.keyset_weight_stats() == {"groups": G, "below_quorum": 0, "launches": launches, "tables": 1}
            ks.close()
        finally:
            e.close()
    assert res[0] == res[1] == res[2]


class Quorum:
    """70 keys, 2 columns, 41 groups: below quorum, reaching and verifying, reaching and failing"""

    def __init__(self, eng, M):
        self.dst = dst = M.DEFAULT_DST
        self.n, self.G = n, G = 70, 41
        rnd = random.Random(17)
        self.com = com = Committee(eng, n, 43)
        at = com.at
        good = [i for i in range(n) if i not in com.unsignable and i != at["ident"]]
        self.cols = [[1] * n, [(1 << 32) + i for i in range(n)]]
        self.min_weight = [30, 30 << 32]
        rows = []
        for g in range(G):
            k = 12 if g % 3 == 0 else 40                                # a third of the groups far below the quorum
            rows.append(set(rnd.sample(good, k)))
        self.fails = {"tampered": 1, "ident_sig": 4, "bad_key": 7, "ident_key_short": 10}
        rows[7] = set(rnd.sample(good, 39)) | {at["off"]}               # 40 bits but 39 count, and the row is invalid
        rows[10] = set(rnd.sample(good, 29)) | {at["ident"]}            # 30 bits of which the identity key weighs nothing: below
        self.rows = rows
        self.sel = [row_of(r, n) for r in rows]
        self.msgs = [b"quorum %d" % g for g in range(G)]
        sigs = sign_rows(eng, com, rows, self.msgs, dst)
        self.msgs[1] += b"!"
        sigs[64 * 4:64 * 5] = IDENT1
        self.sigs = bytes(sigs)

    def expected(self, valid, min_weight):
        w = expect(self.cols, self.rows, valid)
        return w, [all(x >= m for x, m in zip(wg, min_weight)) for wg in w]


@pytest.fixture(scope="module")
def Q(eng, M):
    return Quorum(eng, M)


@pytest.mark.parametrize("chunk", [None, "512"])
def test_quorum_verify(M, Q, monkeypatch, chunk):
    n, G = Q.n, Q.G
    e = fresh_engine(M, monkeypatch, chunk)
    try:
        ks = M.KeySet(e, Q.com.pks, n)
        ks.set_weights(Q.cols)
        valid = bits_of(ks.valid_bitmap(), n)
        parent = e.keyset_fast_aggregate_verify_batch(ks, Q.sel, Q.msgs, Q.sigs, Q.dst)
        pbits = bits_of(parent, G)
        w, reach = Q.expected(valid, Q.min_weight)
        # the shape of the case
        below = [g for g in range(G) if not reach[g]]
        assert len(below) >= G // 3 + 1 and 10 in below and len(Q.rows[10]) == 30
        assert sum(1 for g in range(G) if reach[g] and pbits[g]) >= G // 3 + 1
        assert all(reach[g] and not pbits[g] for g in (1, 4, 7)) and sum(pbits[g] for g in below) >= 10
        s0, t0 = e.keyset_stats(), e.keyset_weight_stats()
        bm, wout = e.keyset_quorum_verify_batch(ks, Q.sel, Q.msgs, Q.sigs, Q.min_weight, Q.dst)
        s1, t1 = e.keyset_stats(), e.keyset_weight_stats()
        assert bits_of(bm, G) == [reach[g] and pbits[g] for g in range(G)]
        assert wout.tolist() == w and wout.tolist() == e.keyset_weight_batch(ks, Q.sel).tolist()
        assert s1["groups"] - s0["groups"] == G - len(below)
        assert t1["groups"] - t0["groups"] == G and t1["below_quorum"] - t0["below_quorum"] == len(below)
        assert t1["launches"] - t0["launches"] == (6 if chunk else 1)
        # every group reaches: the parent's bitmap, every group summed
        for mw in ([12, 0], [0, 0], [1, 1]):
            s0, t0 = e.keyset_stats(), e.keyset_weight_stats()
            bm, wout = e.keyset_quorum_verify_batch(ks, Q.sel, Q.msgs, Q.sigs, mw, Q.dst)
            assert bm == parent and wout.tolist() == w
            assert e.keyset_stats()["groups"] - s0["groups"] == G and e.keyset_weight_stats()["below_quorum"] == t0["below_quorum"]
        # none reaches: nothing summed, nothing paired
        s0, t0 = e.keyset_stats(), e.keyset_weight_stats()
        bm, wout = e.keyset_quorum_verify_batch(ks, Q.sel, Q.msgs, Q.sigs, [41, 0], Q.dst)
        assert bm == bytes((G + 7) // 8) and wout.tolist() == w
        assert e.keyset_stats() == s0 and e.keyset_weight_stats()["below_quorum"] - t0["below_quorum"] == G
        # another rule on the same inputs: the first group below, the last one reaching, the row with the bad key below now
        mw = [40, 0]
        only = [g for g in range(G) if w[g][0] >= 40]
        bm, _ = e.keyset_quorum_verify_batch(ks, Q.sel, Q.msgs, Q.sigs, mw, Q.dst)
        assert 0 not in only and 7 not in only and G - 1 in only and bits_of(bm, G) == [g in only and pbits[g] for g in range(G)]
        ks.close()
    finally:
        e.close()


def test_call_sequences_on_one_context(M, Q):
    """a weight call, a quorum call and an existing verify call on one context, in two orders: each result equals the same call
    on a fresh context"""
    n = Q.n

    def weigh(e, ks):
        return e.keyset_weight_batch(ks, Q.sel).tolist()

    def quorum(e, ks):
        bm, w = e.keyset_quorum_verify_batch(ks, Q.sel, Q.msgs, Q.sigs, Q.min_weight, Q.dst)
        return bm, w.tolist()

    def verify(e, ks):
        return e.keyset_fast_aggregate_verify_batch(ks, Q.sel, Q.msgs, Q.sigs, Q.dst)

    def run(seq):
        e = M.Engine(0)
        try:
            ks = M.KeySet(e, Q.com.pks, n)
            ks.set_weights(Q.cols)
            out = [f(e, ks) for f in seq]
            ks.close()
            return out
        finally:
            e.close()

    alone = {f: run([f])[0] for f in (weigh, quorum, verify)}
    for seq in ([weigh, quorum, verify, quorum, weigh], [verify, quorum, weigh, verify, quorum]):
        assert run(seq) == [alone[f] for f in seq]


def test_argument_errors(eng, M):
    lib, ctx = eng._lib, eng._ctx
    n = 13                                                              # rows of 2 bytes, 3 padding bits
    com = Committee(eng, n, 44)
    dst = b"TEST"
    rows = [{0, 1, 12}, set(range(n)), {5}]
    msgs = [b"a", b"bc", b"def"]
    sigs = np.frombuffer(bytes(sign_rows(eng, com, rows, msgs, dst)), dtype=np.uint8)
    sel = np.frombuffer(b"".join(row_of(r, n) for r in rows), dtype=np.uint8).copy()
    data = np.frombuffer(b"".join(msgs), dtype=np.uint8)
    off = np.array([0, 1, 3, 6], dtype=np.uint64)
    u8, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
    P = lambda a: a.ctypes.data_as(u8)
    Q8 = lambda a: a.ctypes.data_as(u64)
    wts = np.array([list(range(1, n + 1)), [5] * n], dtype=np.uint64)
    out = np.zeros(6, dtype=np.uint64); tot = np.zeros(8, dtype=np.uint64); bm = np.zeros(1, dtype=np.uint8)
    mw = np.array([2, 5], dtype=np.uint64)
    ks = M.KeySet(eng, com.pks, n)
    h = ks._h
    try:
        def setw(c=ctx, k=h, w=Q8(wts), nc=2):
            return lib.blsbn254_keyset_set_weights(c, k, w, ctypes.c_size_t(nc))

        def weigh(c=ctx, k=h, s=P(sel), g=3, o=Q8(out)):
            return lib.blsbn254_keyset_weight_batch(c, k, s, ctypes.c_size_t(g), o)

        def quorum(c=ctx, k=h, s=P(sel), m=P(data), of=Q8(off), sig=P(sigs), g=3, d=dst, dl=4, mn=Q8(mw), wo=Q8(out), b=P(bm)):
            return lib.blsbn254_keyset_quorum_verify_batch(c, k, s, m, of, sig, ctypes.c_size_t(g), d, ctypes.c_size_t(dl), mn, wo, b)

        # a handle without a table
        assert weigh() == E_ARG and b"no weights" in lib.blsbn254_last_error(ctx) and quorum() == E_ARG
        assert lib.blsbn254_keyset_total_weight(ctx, h, Q8(tot)) == E_ARG
        with pytest.raises(M.Bn254Error):
            ks.total_weight()
        for kw in ({"c": None}, {"k": None}, {"w": None}, {"nc": 0}, {"nc": 9}):
            assert setw(**kw) == E_ARG, kw
        assert setw() == 0
        assert lib.blsbn254_keyset_total_weight(ctx, h, Q8(tot)) == 0 and tot.tolist()[:2] == [91, 65]
        assert lib.blsbn254_keyset_total_weight(ctx, h, None) == E_ARG and lib.blsbn254_keyset_total_weight(None, h, Q8(tot)) == E_ARG
        # a column that overflows: refused, and the table is the one before
        over = wts.copy(); over[1, 0] = M64 - 59                        # 5 * 12 + 2^64 - 60 = 2^64
        assert setw(w=Q8(over)) == E_ARG and b"column 1" in lib.blsbn254_last_error(ctx)
        over[1, 0] -= 1                                                 # 2^64 - 1: accepted
        assert setw(w=Q8(over)) == 0 and lib.blsbn254_keyset_total_weight(ctx, h, Q8(tot)) == 0 and tot.tolist()[:2] == [91, M64]
        over[1, 0] += 1
        assert setw(w=Q8(over)) == E_ARG and lib.blsbn254_keyset_total_weight(ctx, h, Q8(tot)) == 0 and tot.tolist()[:2] == [91, M64]
        assert setw() == 0
        assert weigh() == 0 and out.tolist() == [16, 15, 91, 65, 6, 5]
        assert quorum() == 0 and bm[0] == 7 and out.tolist() == [16, 15, 91, 65, 6, 5]
        for name in ("c", "k", "s", "o"):
            assert weigh(**{name: None}) == E_ARG, name
        for name in ("c", "k", "s", "of", "sig", "d", "mn", "wo", "b"):
            assert quorum(**{name: None}) == E_ARG, name
        assert weigh(g=0) == 0 and quorum(g=0) == 0 and weigh(g=0, s=None, o=None) == 0
        e2 = M.Engine(0)                                                # a key set that belongs to another context
        try:
            assert weigh(c=e2._ctx) == E_ARG and quorum(c=e2._ctx) == E_ARG and setw(c=e2._ctx) == E_ARG
        finally:
            e2.close()
        sel[2 * 1 + 1] ^= 1 << 6                                        # a padding bit
        assert weigh() == E_ARG and b"row 1" in lib.blsbn254_last_error(ctx) and quorum() == E_ARG
        sel[2 * 1 + 1] ^= 1 << 6
        bad_off = np.array([0, 3, 1, 6], dtype=np.uint64)
        assert quorum(of=Q8(bad_off)) == E_ARG
        assert lib.blsbn254_keyset_weight_stats(ctx, None) == E_ARG and lib.blsbn254_keyset_weight_stats(None, (ctypes.c_uint64 * 4)()) == E_ARG
        mw[0] = 7                                                       # the last row is below: after the errors, the context still serves
        assert quorum() == 0 and bm[0] == 3
        with pytest.raises(ValueError):
            eng.keyset_quorum_verify_batch(ks, [bytes(2)], [b"a"], bytes(64), [1], dst)
        with pytest.raises(ValueError):
            ks.set_weights([[1] * (n - 1)])
    finally:
        ks.close()
