"""GPU tests (MI355X) of the entry points that take compressed encodings: the inflate primitives against the oracle's
decompression (or the marker), and every fused call against the uncompressed call on the inflate outputs -- byte equality
throughout.  Expected bits of the bad tuples are stated here, not taken from the calls under test."""
import ctypes
import random

import numpy as np
import pytest

from tests import compressed_cases as cc
from tests import synth
from tests.gpu_support import eng, M
from tests.helpers import b32, bits_of, IDENT1

pytestmark = pytest.mark.gpu
E_ARG = -1
SEED = bytes(range(32))
u8 = ctypes.POINTER(ctypes.c_uint8)
u64 = ctypes.POINTER(ctypes.c_uint64)


def split(b, w):
    return [b[w * i:w * i + w] for i in range(len(b) // w)]


# ---------------------------------------------------------------- inflate parity
@pytest.fixture(scope="module")
def cases(oracle):
    """per group: (classes, {encoding: (expected bytes, status)}) -- the oracle is asked once per distinct encoding"""
    out = {}
    for g, classes, expect in (("g1", cc.g1_classes(oracle), cc.g1_expect), ("g2", cc.g2_classes(oracle), cc.g2_expect)):
        out[g] = (classes, {c: expect(oracle, c) for members in classes.values() for c in members})
    return out


@pytest.mark.parametrize("n", [257, 1, 63, 64, 65])
@pytest.mark.parametrize("group", ["g1", "g2"])
def test_inflate_equals_the_oracle_or_the_marker(eng, cases, group, n):
    classes, expect = cases[group]
    w = 32 if group == "g1" else 64
    inflate, decompress = (eng.g1_inflate_batch, eng.g1_decompress_batch) if group == "g1" else (eng.g2_inflate_batch, eng.g2_decompress_batch)
    enc = cc.mixed(classes, n, 100 + n)
    assert len(enc) == n
    if n == 257:
        assert set(enc) == set(expect)                                # every member of every class
    out, status = inflate(b"".join(enc), n)
    assert len(out) == 2 * w * n and len(status) == n
    assert split(out, 2 * w) == [expect[c][0] for c in enc]
    assert list(status) == [expect[c][1] for c in enc]
    good = [c for c in enc if expect[c][1]]
    if good:
        assert decompress(b"".join(good), len(good)) == b"".join(o for o, s in zip(split(out, 2 * w), status) if s)
    if n == 257:
        assert 0 < len(good) < n


# ---------------------------------------------------------------- verify
class Batch:
    """67 tuples over a pool of 5 keys, signed by the engine, compressed by the oracle, with the seven kinds of bad tuple"""
    N, POOL = 67, 5
    BAD = {"wrong sig": 3, "sig no point": 11, "sig x>=p": 20, "key no point": 29, "key non-subgroup": 38, "sig identity": 47, "key identity": 66}

    def __init__(self, eng, oracle, dst):
        n = self.N
        sks = [synth.sk_of(700 + k) for k in range(self.POOL)]
        pool = split(eng.sk_to_pk_batch(b"".join(map(b32, sks)), self.POOL), 128)
        pool_c = [oracle.g2_compress(pk) for pk in pool]
        self.msgs = [b"compressed tuple %d" % i for i in range(n)]
        sigs = split(eng.sign_batch(b"".join(b32(sks[i % self.POOL]) for i in range(n)), self.msgs, dst), 64)
        assert sigs[0] == oracle.sign(sks[0], self.msgs[0], dst)
        pks_c = [pool_c[i % self.POOL] for i in range(n)]
        sigs_c = [oracle.g1_compress(s) for s in sigs]
        rnd = random.Random(9)
        bad = self.BAD
        sigs_c[bad["wrong sig"]] = sigs_c[bad["wrong sig"] + self.POOL]           # the same key's signature of another message
        sigs_c[bad["sig no point"]] = cc.g1_no_point(oracle, rnd, 1)[0]
        sigs_c[bad["sig x>=p"]] = cc.be(cc.P + 5)
        pks_c[bad["key no point"]] = cc.g2_no_point(oracle, rnd, 1)[0]
        pks_c[bad["key non-subgroup"]] = oracle.g2_compress(synth.NON_SUBGROUP_PK)
        sigs_c[bad["sig identity"]] = bytes(32)
        pks_c[bad["key identity"]] = bytes(64)
        self.pks_c, self.sigs_c = pks_c, sigs_c
        self.want = synth.bitmap_of([i not in bad.values() for i in range(n)])


@pytest.fixture(scope="module")
def batch(eng, oracle, M):
    return Batch(eng, oracle, M.DEFAULT_DST)


def test_verify_compressed_equals_verify_on_the_inflated_operands(eng, oracle, M, batch):
    dst, n = M.DEFAULT_DST, batch.N
    pks_c, sigs_c = b"".join(batch.pks_c), b"".join(batch.sigs_c)
    pks, pst = eng.g2_inflate_batch(pks_c, n)
    sigs, sst = eng.g1_inflate_batch(sigs_c, n)
    bad = batch.BAD
    assert [i for i in range(n) if not pst[i]] == [bad["key no point"]]
    assert [i for i in range(n) if not sst[i]] == [bad["sig no point"], bad["sig x>=p"]]
    assert split(pks, 128)[bad["key non-subgroup"]] == synth.NON_SUBGROUP_PK
    try:
        for auto in (1, 0):                                            # off: the exact per-tuple path at this size
            eng.set_auto_prepare(auto)
            before = eng.path_stats()
            got = eng.verify_batch_compressed(pks_c, batch.msgs, sigs_c, dst)
            after = eng.path_stats()
            assert got == eng.verify_batch(pks, batch.msgs, sigs, dst) == batch.want, auto
            assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if auto else (0, 1))      # (prepared, exact) chunks
    finally:
        eng.set_auto_prepare(1)
    assert eng.verify_batch_rlc_compressed(pks_c, batch.msgs, sigs_c, dst, seed=SEED) == batch.want
    assert eng.verify_batch_rlc(pks, batch.msgs, sigs, dst, seed=SEED) == batch.want
    # n == 1: a good tuple, then one whose signature does not inflate
    assert eng.verify_batch_compressed(batch.pks_c[0], batch.msgs[:1], batch.sigs_c[0], dst) == b"\x01"
    i = bad["sig no point"]
    assert eng.verify_batch_compressed(batch.pks_c[i], [batch.msgs[i]], batch.sigs_c[i], dst) == b"\x00"


# ---------------------------------------------------------------- key set
class Set70:
    """70 keys (three 32-key words, the last partial) with a key that has no point, an identity and the non-subgroup key; proofs
    of possession with one wrong proof and one that does not inflate; nine rows and their aggregate signatures"""
    N = 70
    BAD_KEYS = {"no point": 7, "identity": 40, "non-subgroup": 66}
    WRONG_PROOF, NO_PROOF = 12, 50

    def __init__(self, eng, oracle, dst):
        n = self.N
        rnd = random.Random(70)
        self.sks = [synth.sk_of(900 + k) for k in range(n)]
        keys = split(eng.sk_to_pk_batch(b"".join(map(b32, self.sks)), n), 128)
        self.pks_c = [oracle.g2_compress(k) for k in keys]
        self.pks_c[self.BAD_KEYS["no point"]] = cc.g2_no_point(oracle, rnd, 1)[0]
        self.pks_c[self.BAD_KEYS["identity"]] = bytes(64)
        self.pks_c[self.BAD_KEYS["non-subgroup"]] = oracle.g2_compress(synth.NON_SUBGROUP_PK)
        proofs = split(eng.pop_prove_batch(b"".join(map(b32, self.sks)), n), 64)
        self.proofs_c = [oracle.g1_compress(p) for p in proofs]
        self.proofs_c[self.WRONG_PROOF] = self.proofs_c[self.WRONG_PROOF + 1]
        self.proofs_c[self.NO_PROOF] = cc.g1_no_point(oracle, rnd, 1)[0]
        bad = set(self.BAD_KEYS.values())
        good = [i for i in range(n) if i not in bad]
        clean = [i for i in good if i not in (self.WRONG_PROOF, self.NO_PROOF)]
        self.rows = [set(), set(range(n)), {5}, set(clean[:48]), {3, self.BAD_KEYS["no point"], 9}, set(good), {self.WRONG_PROOF, 1, 2},
                     set(clean[10:20]), set(clean[-5:])]
        self.names = {"empty": 0, "full": 1, "one": 2, "more than half": 3, "bad key": 4, "good": 5, "wrong proof": 6, "no sig": 7, "tail": 8}
        self.sel = [bytes(np.packbits(np.array([i in r for i in range(n)], dtype=np.uint8), bitorder="little")) for r in self.rows]
        self.msgs = [b"compressed row %d" % g for g in range(len(self.rows))]
        sigs = []
        for g, r in enumerate(self.rows):
            signers = sorted(r - bad)
            if not signers:
                sigs.append(IDENT1)
                continue
            ss = eng.sign_batch(b"".join(b32(self.sks[i]) for i in signers), [self.msgs[g]] * len(signers), dst)
            sigs.append(eng.aggregate_sigs(ss, len(signers)))
        self.sigs_c = [oracle.g1_compress(s) for s in sigs]
        self.sigs_c[self.names["no sig"]] = cc.g1_no_point(oracle, rnd, 1)[0]


@pytest.fixture(scope="module")
def set70(eng, oracle, M):
    return Set70(eng, oracle, M.DEFAULT_DST)


def keyset_calls(eng, ks, s, sigs, sigs_c, dst):
    return (ks.valid_bitmap(), eng.keyset_sum_batch(ks, s.sel), eng.keyset_fast_aggregate_verify_batch(ks, s.sel, s.msgs, sigs, dst),
            eng.keyset_fast_aggregate_verify_batch_compressed(ks, s.sel, s.msgs, sigs_c, dst))


@pytest.mark.parametrize("with_proofs", [False, True])
def test_compressed_key_set_equals_the_set_of_the_inflated_keys(eng, M, set70, with_proofs):
    dst, s, n = M.DEFAULT_DST, set70, set70.N
    pks_c, proofs_c, sigs_c = b"".join(s.pks_c), b"".join(s.proofs_c), b"".join(s.sigs_c)
    pks, pst = eng.g2_inflate_batch(pks_c, n)
    proofs, qst = eng.g1_inflate_batch(proofs_c, n)
    sigs, sst = eng.g1_inflate_batch(sigs_c, len(s.rows))
    assert [i for i in range(n) if not pst[i]] == [s.BAD_KEYS["no point"]] and [i for i in range(n) if not qst[i]] == [s.NO_PROOF]
    assert [g for g in range(len(s.rows)) if not sst[g]] == [s.names["no sig"]]
    kw = dict(proofs=proofs, pop_dst=M.POP_DST) if with_proofs else {}
    kw_c = dict(proofs=proofs_c, pop_dst=M.POP_DST) if with_proofs else {}
    plain = M.KeySet(eng, pks, n, **kw)
    comp = M.KeySet(eng, pks_c, n, compressed=True, **kw_c)
    try:
        assert comp.checked() == with_proofs and comp.count() == n
        got, want = keyset_calls(eng, comp, s, sigs, sigs_c, dst), keyset_calls(eng, plain, s, sigs, sigs_c, dst)
    finally:
        plain.close(); comp.close()
    assert got == want
    assert got[3] == got[2]                                            # compressed signatures: the uncompressed call on the inflated ones
    # what the equalities rest on, stated independently: the bad keys, the failed proofs, the rows they spoil
    bad = set(s.BAD_KEYS.values()) | ({s.WRONG_PROOF, s.NO_PROOF} if with_proofs else set())
    assert got[0] == synth.bitmap_of([i not in bad for i in range(n)])
    undec = bad if with_proofs else {s.BAD_KEYS["no point"]}           # a sum fails on a key that does not decode; with proofs, on every key whose proof fails
    assert list(got[1][1]) == [0 if r & undec else 1 for r in s.rows]
    ok = [bool(r) and not (r & bad) and g != s.names["no sig"] for g, r in enumerate(s.rows)]
    assert bits_of(got[2], len(s.rows)) == ok and any(ok)


# ---------------------------------------------------------------- sequences on one context
def test_calls_in_sequence_equal_the_same_calls_on_fresh_contexts(M, oracle, batch, set70):
    """verify_batch -> verify_batch_compressed -> g1_decompress_batch -> compressed KeySet with proofs -> its compressed verify ->
    verify_batch on ONE context, each against the same call on a context of its own: the inflated bytes reuse in_a / in_b."""
    dst, s = M.DEFAULT_DST, set70
    n2 = 40
    pks_c, sigs_c = b"".join(batch.pks_c), b"".join(batch.sigs_c)
    points = b"".join(cc.g1_points(oracle, 30))
    set_pks_c, set_proofs_c, row_sigs_c = b"".join(s.pks_c), b"".join(s.proofs_c), b"".join(s.sigs_c)

    def with_set(e, f):
        ks = M.KeySet(e, set_pks_c, s.N, proofs=set_proofs_c, compressed=True)
        try:
            return f(e, ks)
        finally:
            ks.close()

    ref = M.Engine(0)
    try:
        pks, _ = ref.g2_inflate_batch(pks_c, batch.N)
        sigs, _ = ref.g1_inflate_batch(sigs_c, batch.N)
    finally:
        ref.close()
    steps = [
        lambda e: e.verify_batch(pks, batch.msgs, sigs, dst),
        lambda e: e.verify_batch_compressed(pks_c[:64 * n2], batch.msgs[:n2], sigs_c[:32 * n2], dst),
        lambda e: e.g1_decompress_batch(points, 30),
        lambda e: with_set(e, lambda e, ks: (ks.valid_bitmap(), e.keyset_fast_aggregate_verify_batch_compressed(ks, s.sel, s.msgs, row_sigs_c, dst))),
        lambda e: e.verify_batch(pks, batch.msgs, sigs, dst),
    ]
    one = M.Engine(0)
    try:
        got = [f(one) for f in steps]
    finally:
        one.close()
    want = []
    for f in steps:
        e = M.Engine(0)
        try:
            want.append(f(e))
        finally:
            e.close()
    assert got == want
    assert got[0] == got[4] == batch.want and got[1] == batch.want[:n2 // 8]


# ---------------------------------------------------------------- arguments
def test_arguments(M, eng, batch, set70):
    lib, ctx, dst = eng._lib, eng._ctx, M.DEFAULT_DST
    P = lambda a: a.ctypes.data_as(u8)
    n = 3
    pk = np.frombuffer(b"".join(batch.pks_c[:n]), dtype=np.uint8).copy()
    sg = np.frombuffer(b"".join(batch.sigs_c[:n]), dtype=np.uint8).copy()
    data, off = M.engine.pack_messages(batch.msgs[:n])
    ms = np.frombuffer(data, dtype=np.uint8).copy()
    out = np.full(128 * n, 0x5a, dtype=np.uint8); st = np.full(n, 0x5a, dtype=np.uint8); bm = np.full(1, 0x5a, dtype=np.uint8)
    seed = np.frombuffer(SEED, dtype=np.uint8).copy()

    def untouched():
        return bool((out == 0x5a).all() and (st == 0x5a).all() and (bm == 0x5a).all())

    def inf(fn, c=ctx, i=P(pk), k=n, o=P(out), t=P(st)):
        return fn(c, i, ctypes.c_size_t(k), o, t)

    for fn in (lib.blsbn254_g1_inflate_batch, lib.blsbn254_g2_inflate_batch):
        for name in ("c", "i", "o", "t"):
            assert inf(fn, **{name: None}) == E_ARG and untouched(), name
        assert inf(fn, k=0) == 0 and inf(fn, k=0, i=None, o=None, t=None) == 0 and untouched()

    def ver(c=ctx, p=P(pk), m=P(ms), of=off.ctypes.data_as(u64), s=P(sg), k=n, d=dst, dl=len(dst), b=P(bm)):
        return lib.blsbn254_verify_batch_compressed(c, p, m, of, s, ctypes.c_size_t(k), d, ctypes.c_size_t(dl), b)

    def rlc(c=ctx, p=P(pk), m=P(ms), of=off.ctypes.data_as(u64), s=P(sg), k=n, d=dst, dl=len(dst), b=P(bm)):
        return lib.blsbn254_verify_batch_rlc_compressed(c, p, m, of, s, ctypes.c_size_t(k), d, ctypes.c_size_t(dl), P(seed), b)

    for f in (ver, rlc):
        for name in ("c", "p", "of", "s", "d", "b"):
            assert f(**{name: None}) == E_ARG and untouched(), name
        assert f(k=0) == 0 and f(k=0, p=None, s=None, b=None) == 0 and untouched()
    assert ver() == 0 and bm[0] == 7
    bm[:] = 0x5a
    assert rlc() == 0 and bm[0] == 7
    bm[:] = 0x5a

    s = set70
    kp = np.frombuffer(b"".join(s.pks_c), dtype=np.uint8).copy()
    pr = np.frombuffer(b"".join(s.proofs_c), dtype=np.uint8).copy()

    def create(c=ctx, p=P(kp), q=P(pr), k=s.N, d=M.POP_DST, dl=len(M.POP_DST), out_h=True):
        h = ctypes.c_void_p(0x5a5a)
        return lib.blsbn254_keyset_create_compressed(c, p, q, ctypes.c_size_t(k), d, ctypes.c_size_t(dl), ctypes.byref(h) if out_h else None), h

    for kwargs in (dict(c=None), dict(p=None), dict(out_h=False), dict(d=None), dict(k=0), dict(k=65537)):
        rc, h = create(**kwargs)
        assert rc == E_ARG and (not h.value or "out_h" in kwargs), kwargs
    rc, h = create(q=None, d=None, dl=0)                                # without proofs the tag is not looked at
    assert rc == 0 and lib.blsbn254_keyset_checked(h) == 0
    sel = np.frombuffer(b"".join(s.sel[2:5]), dtype=np.uint8).copy()
    rs = np.frombuffer(b"".join(s.sigs_c[2:5]), dtype=np.uint8).copy()
    rdata, roff = M.engine.pack_messages(s.msgs[2:5])
    rm = np.frombuffer(rdata, dtype=np.uint8).copy()

    def fav(c=ctx, k=h, r=P(sel), m=P(rm), of=roff.ctypes.data_as(u64), sig=P(rs), g=3, d=dst, dl=len(dst), b=P(bm)):
        return lib.blsbn254_keyset_fast_aggregate_verify_batch_compressed(c, k, r, m, of, sig, ctypes.c_size_t(g), d, ctypes.c_size_t(dl), b)

    try:
        for name in ("c", "k", "r", "of", "sig", "d", "b"):
            assert fav(**{name: None}) == E_ARG and untouched(), name
        assert fav(g=0) == 0 and fav(g=0, r=None, sig=None, b=None) == 0 and untouched()
        e2 = M.Engine(0)                                                # a key set that belongs to another context
        try:
            assert fav(c=e2._ctx) == E_ARG and untouched()
        finally:
            e2.close()
        assert fav() == 0 and bm[0] == 0b011                             # rows "one" and "more than half" hold, "bad key" does not
    finally:
        lib.blsbn254_keyset_destroy(h)
