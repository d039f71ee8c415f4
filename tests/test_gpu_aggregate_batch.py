"""GPU tests (MI355X) of the aggregate verify over ragged groups of (key, message) pairs (blsbn254_aggregate_verify_batch): bit g
must be what blsbn254_aggregate_verify gives on group g alone, which is checked against the CPU oracle's aggregate_verify; one
damaged member clears exactly its group's bit; offsets need not start at 0; the result equals the host composition
hash_to_g1_batch + pairing_check_batch; every size class, launch form setting and chunking gives the same bitmap; the call keeps
its result in a sequence with asynchronous verify calls under another tag; a large batch; the argument errors."""
import ctypes
import random

import numpy as np
import pytest

from tests import synth
from tests.gpu_support import eng, M
from tests.helpers import bits_of, IDENT1, IDENT2, offsets_u64

pytestmark = pytest.mark.gpu
R = synth.R
E_ARG = -1


def oracle_verify(oracle, pks, msgs, sig, dst):
    """the oracle's aggregate_verify as a boolean: a point it refuses to decode makes the aggregate invalid"""
    if not msgs:
        return False
    try:
        return oracle.aggregate_verify(pks, msgs, sig, dst)
    except Exception:
        return False


class Groups:
    """sizes[g] tuples of synth.make_batch per group (64 signed tuples tiled: a group may repeat a tuple, which keeps it valid),
    the aggregate of each group's signatures from the oracle (an empty group: the first tuple's signature)"""
    def __init__(self, oracle, sizes, dst, uniq=64):
        n = sum(sizes)
        pks, msgs, sigs, _ = synth.make_batch(oracle, max(n, 1), dst, pool=8, uniq=min(max(n, 1), uniq))
        self.dst, self.sizes = dst, list(sizes)
        self.keys, self.msgs, self.sigs, self.tuple_sigs = [], [], [], []
        pos = 0
        for k in sizes:
            self.keys.append([pks[128 * i:128 * i + 128] for i in range(pos, pos + k)])
            self.msgs.append(list(msgs[pos:pos + k]))
            ts = [sigs[64 * i:64 * i + 64] for i in range(pos, pos + k)]
            self.tuple_sigs.append(ts)
            self.sigs.append(oracle.aggregate_sigs(b"".join(ts), k) if k else sigs[:64])
            pos += k

    def flip_message(self, g, j=0):
        m = self.msgs[g][j]
        self.msgs[g][j] = bytes([m[0] ^ 1]) + m[1:]

    def key_sets(self):
        return [b"".join(k) for k in self.keys]

    def run(self, e):
        return e.aggregate_verify_batch(self.key_sets(), self.msgs, b"".join(self.sigs), self.dst)

    def single(self, e, g):
        return e.aggregate_verify(b"".join(self.keys[g]), self.msgs[g], self.sigs[g], self.dst)

    def oracle_bit(self, oracle, g):
        return oracle_verify(oracle, b"".join(self.keys[g]), self.msgs[g], self.sigs[g], self.dst)


# ---------------------------------------------------------------- 1. small ragged batch
def test_small_ragged_batch(eng, oracle, M):
    sizes = [1, 2, 3, 4, 7, 33, 0, 2]
    G = Groups(oracle, sizes, M.DEFAULT_DST)
    G.flip_message(1, 1)
    G.flip_message(4, 6)
    G.sigs[7] = oracle.g1_add(G.sigs[7], oracle.g1_generator())
    bits = bits_of(G.run(eng), len(sizes))
    for g in range(len(sizes)):
        assert bits[g] == G.single(eng, g), g
        assert bits[g] == G.oracle_bit(oracle, g), g
    assert bits == [True, False, True, True, False, True, False, False]
    assert any(bits) and not all(bits)


# ---------------------------------------------------------------- 2. damage clears exactly its group's bit
def test_damage_clears_exactly_its_groups_bit(eng, oracle, M):
    n_g = 17
    G = Groups(oracle, [3] * n_g, M.DEFAULT_DST)
    assert bits_of(G.run(eng), n_g) == [True] * n_g                 # all valid before the damage
    bad_x = b"\xff" * 32
    G.flip_message(1, 2)                                              # a flipped message byte
    G.sigs[2], G.sigs[3] = G.sigs[3], G.sigs[2]                       # two groups' signatures swapped
    G.sigs[4] = IDENT1                                                # an identity signature
    G.sigs[5] = G.sigs[5][:63] + bytes([G.sigs[5][63] ^ 1])           # an off-curve signature
    G.sigs[6] = bad_x + G.sigs[6][32:]                                # an undecodable signature (x >= p)
    G.keys[8][1] = IDENT2                                             # an identity key
    G.keys[9][0] = bad_x + G.keys[9][0][32:]                          # an undecodable key
    G.keys[10][2] = G.keys[10][2][:127] + bytes([G.keys[10][2][127] ^ 1])   # an off-curve key
    G.keys[11][1] = synth.NON_SUBGROUP_PK                             # on the twist, outside the r-torsion
    G.keys[12], G.msgs[12] = [], []                                   # an empty group (its signature stays a valid point)
    # group 14 would cancel to 1 but for an identity key: the key is the identity and the signature leaves that tuple out
    G.keys[14][1] = IDENT2
    G.sigs[14] = oracle.aggregate_sigs(G.tuple_sigs[14][0] + G.tuple_sigs[14][2], 2)
    damaged = {1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 14}
    want = [g not in damaged for g in range(n_g)]
    bits = bits_of(G.run(eng), n_g)
    for g in range(n_g):
        assert G.single(eng, g) == want[g], g
        assert G.oracle_bit(oracle, g) == want[g], g
    assert bits == want
    # group 14 without the identity key (two pairs, the same signature) holds: only the key's flag makes it invalid
    assert oracle.aggregate_verify(G.keys[14][0] + G.keys[14][2], [G.msgs[14][0], G.msgs[14][2]], G.sigs[14], M.DEFAULT_DST) is True


# ---------------------------------------------------------------- 3. offsets need not start at 0
def test_group_offsets_need_not_start_at_zero(eng, oracle, M):
    dst = M.DEFAULT_DST
    G = Groups(oracle, [2, 2, 0, 3, 1], dst)
    G.flip_message(3, 0)
    keys = b"".join(G.key_sets()); msgs = [m for ms in G.msgs for m in ms]
    goff = offsets_u64(G.sizes)[1:]                                       # the first group's two pairs belong to no group
    sigs = b"".join(G.sigs[1:])
    want = [True, False, False, True]
    assert bits_of(eng.aggregate_verify_batch_flat(keys, msgs, goff, sigs, dst), 4) == want
    # damage in the leading pairs changes nothing
    keys2 = b"\xff" * 32 + keys[32:128] + IDENT2 + keys[256:]
    msgs2 = [b"other", b""] + msgs[2:]
    assert bits_of(eng.aggregate_verify_batch_flat(keys2, msgs2, goff, sigs, dst), 4) == want
    for g in range(4):
        assert G.single(eng, g + 1) == want[g]


# ---------------------------------------------------------------- 4. the host composition
def test_equals_hash_and_pairing_check_composition(eng, oracle, M):
    dst = M.DEFAULT_DST
    rnd = random.Random(4)
    sizes = [rnd.randint(1, 6) for _ in range(200)]
    G = Groups(oracle, sizes, dst)
    want = []
    for g in range(len(sizes)):
        want.append(g % 4 != 3)
        if not want[g]:
            G.flip_message(g, rnd.randrange(sizes[g]))
    neg_g2 = oracle.g2_mul(oracle.g2_generator(), R - 1)
    H = eng.hash_to_g1_batch([m for ms in G.msgs for m in ms], dst)
    P, Q, pos = [], [], 0
    for g, k in enumerate(sizes):
        P.append(G.sigs[g] + H[64 * pos:64 * (pos + k)])
        Q.append(neg_g2 + b"".join(G.keys[g]))
        pos += k
    comp = eng.pairing_check_batch(b"".join(P), b"".join(Q), offsets_u64([k + 1 for k in sizes]))
    got = G.run(eng)
    assert got == comp
    assert bits_of(got, len(sizes)) == want


# ---------------------------------------------------------------- 5. forms and chunking
ENVS = [{"BLSBN254_WIDE_FE": "0"}, {"BLSBN254_TRI_MAX": "0"}, {"BLSBN254_WIDE_FE": "0", "BLSBN254_TRI_MAX": "0"}]


def _lanes(sizes):
    return sum((k + 2) // 2 for k in sizes)


def _ragged_groups(oracle, dst, sizes, seed, every=5):
    rnd = random.Random(seed)
    G = Groups(oracle, sizes, dst)
    want = []
    for g, k in enumerate(sizes):
        ok = k > 0 and g % every != every - 1
        if k and not ok:
            G.flip_message(g, rnd.randrange(k))
        want.append(ok)
    return G, want


def _run_forms(M, eng, oracle, monkeypatch, G, want, envs, sample, min_launches=1):
    n_g = len(G.sizes)
    bm = G.run(eng)
    assert bits_of(bm, n_g) == want
    for g in sample:
        assert G.single(eng, g) == want[g], g
    for env in envs:
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            e2 = M.Engine(0)
            try:
                assert e2.aggregate_verify_batch(G.key_sets(), G.msgs, b"".join(G.sigs), G.dst) == bm, env
                st = e2.aggregate_batch_stats()
                print("gpu_aggregate_batch forms: %d groups, %d pairs, env %s: stats %s" % (n_g, sum(G.sizes), env, st))
                # which path ran: every size takes the two-pair lane kernel in this build, none of the small forms
                assert st["groups"] == n_g and st["lanes"] == _lanes(G.sizes) and st["small_calls"] == 0
                assert st["launches"] >= min_launches
            finally:
                e2.close()


def test_up_to_1024_pairs(M, eng, oracle, monkeypatch):
    rnd = random.Random(10)
    sizes = [rnd.randint(1, 5) for _ in range(250)]
    assert sum(sizes) <= 1024
    G, want = _ragged_groups(oracle, M.DEFAULT_DST, sizes, 11)
    _run_forms(M, eng, oracle, monkeypatch, G, want, ENVS, range(0, 250, 25))


def test_up_to_16384_pairs(M, eng, oracle, monkeypatch):
    rnd = random.Random(12)
    sizes = [rnd.randint(1, 4) for _ in range(2500)]
    assert 1024 < sum(sizes) <= 16384
    G, want = _ragged_groups(oracle, M.DEFAULT_DST, sizes, 13)
    _run_forms(M, eng, oracle, monkeypatch, G, want, ENVS, range(4, 2500, 250))


def test_more_than_16384_pairs(M, eng, oracle, monkeypatch):
    rnd = random.Random(14)
    sizes = [rnd.randint(1, 4) for _ in range(8000)]
    assert sum(sizes) > 16384
    G, want = _ragged_groups(oracle, M.DEFAULT_DST, sizes, 15)
    _run_forms(M, eng, oracle, monkeypatch, G, want, ENVS, range(4, 8000, 800))


def test_chunking_straddles_and_exceeds_a_chunk(M, eng, oracle, monkeypatch):
    rnd = random.Random(16)
    sizes = [rnd.randint(1, 150) for _ in range(60)]
    sizes[3:3] = [0, 0]                                               # empty groups in the middle, and at the end
    sizes += [0]
    G, want = _ragged_groups(oracle, M.DEFAULT_DST, sizes, 17, every=4)
    assert any(want) and not all(want)
    _run_forms(M, eng, oracle, monkeypatch, G, want, [{"BLSBN254_CHUNK_LANES": "64"}, {"BLSBN254_CHUNK_LANES": "8"}], range(len(sizes)),
               min_launches=_lanes(sizes) // 64)


def test_one_huge_group_between_small_ones(M, eng, oracle, monkeypatch):
    for seed, bad in ((18, None), (19, 1), (20, 2)):
        G = Groups(oracle, [1, 5000, 2], M.DEFAULT_DST)
        want = [True, True, True]
        if bad is not None:
            G.flip_message(bad, G.sizes[bad] - 1)
            want[bad] = False
        _run_forms(M, eng, oracle, monkeypatch, G, want, [{"BLSBN254_CHUNK_LANES": "512"}], range(3), min_launches=4)
        if bad is None:
            assert G.oracle_bit(oracle, 0) and G.oracle_bit(oracle, 2)


# ---------------------------------------------------------------- 6. call sequences on one context
def test_between_asynchronous_verify_calls_under_another_tag(eng, oracle, M):
    """verify_batch_dev on the asynchronous path under tag A (left pending), aggregate_verify_batch under tag B, verify under tag A
    again: every result equals the same call on a context of its own and the closed form."""
    import torch
    tag_a = M.DEFAULT_DST
    tag_b = tag_a[:-1] + bytes([tag_a[-1] ^ 1])
    n = 4100
    A = synth.make_batch_gpu(eng, oracle, n, tag_a, pool=40, invalid_every=7, spot=6)
    want_a = synth.bitmap_of(A[3])
    G, want_g = _ragged_groups(oracle, tag_b, [random.Random(21).randint(1, 6) for _ in range(300)], 22)
    G_a = Groups(oracle, G.sizes, tag_a)                              # the same groups signed under tag A: all invalid under tag B
    want_bm = synth.bitmap_of(want_g)

    def dev(e, bm):
        e.verify_batch_dev(tA[0].data_ptr(), tA[1].data_ptr(), tA[2].data_ptr(), tA[3].data_ptr(), n, bm.data_ptr(), tag_a)

    tA = synth.dev_batch(M, torch, A[0], A[1], A[2])
    bms = [torch.full_like(tA[4], 0x5a) for _ in range(4)]
    torch.cuda.synchronize()
    fresh = M.Engine(0)
    try:
        assert G.run(fresh) == want_bm
        assert fresh.aggregate_verify_batch(G_a.key_sets(), G_a.msgs, b"".join(G_a.sigs), tag_b) == bytes(len(want_bm))
    finally:
        fresh.close()
    fresh = M.Engine(0)
    try:
        dev(fresh, bms[0]); fresh.synchronize()
        assert bytes(bms[0].cpu().numpy()) == want_a
    finally:
        fresh.close()
    e = M.Engine(0)
    try:
        dev(e, bms[1]); e.synchronize()
        a0, r0 = e.async_stats()
        dev(e, bms[2])                                                # enqueued on the remembered key count: pending
        assert e.async_stats() == (a0 + 1, r0)
        got = G.run(e)                                                # settles it, then stages tag B
        got_a = e.aggregate_verify_batch(G_a.key_sets(), G_a.msgs, b"".join(G_a.sigs), tag_b)
        dev(e, bms[3])
        e.synchronize()
        assert got == want_bm and got_a == bytes(len(want_bm))
        for bm in bms[1:]:
            assert bytes(bm.cpu().numpy()) == want_a
        assert G.run(e) == want_bm
    finally:
        e.close()


# ---------------------------------------------------------------- 7. large batch
def test_large_batch(eng, oracle, M):
    dst = M.DEFAULT_DST
    n_g, per = 1 << 16, 4
    n = n_g * per
    pks, msgs, sigs, exp = synth.make_batch_gpu(eng, oracle, n, dst, pool=1024, invalid_every=64)
    aggs = []
    for g in range(n_g):
        lo = per * g
        ts = [sigs[64 * i:64 * i + 64] for i in range(lo, lo + per)]
        if not all(exp[lo:lo + per]):                                 # leave out a signature that does not decode or is off the curve
            ts = [s for s in ts if oracle.g1_check_batch(s, 1)[0] & 1]
        aggs.append(oracle.aggregate_sigs(b"".join(ts), len(ts)))
    want = [g % 16 != 15 for g in range(n_g)]
    assert want == [all(exp[per * g:per * g + per]) for g in range(n_g)]
    for g in range(1024):
        lo = per * g
        assert oracle_verify(oracle, pks[128 * lo:128 * (lo + per)], msgs[lo:lo + per], aggs[g], dst) == want[g], g
    key_sets = [pks[128 * per * g:128 * per * (g + 1)] for g in range(n_g)]
    msg_sets = [msgs[per * g:per * g + per] for g in range(n_g)]
    got = eng.aggregate_verify_batch(key_sets, msg_sets, b"".join(aggs), dst)
    assert got == synth.bitmap_of(want)


# ---------------------------------------------------------------- 8. argument errors
def test_argument_errors(eng, oracle, M):
    lib, ctx = eng._lib, eng._ctx
    u8 = ctypes.POINTER(ctypes.c_uint8); u64 = ctypes.POINTER(ctypes.c_uint64)
    dst = M.DEFAULT_DST
    G = Groups(oracle, [2, 2], dst)
    pk = np.frombuffer(b"".join(G.key_sets()), dtype=np.uint8); ms = np.frombuffer(b"".join(m for x in G.msgs for m in x), dtype=np.uint8)
    sg = np.frombuffer(b"".join(G.sigs), dtype=np.uint8); d = np.frombuffer(dst, dtype=np.uint8)
    off = np.arange(0, 32 * 5, 32, dtype=np.uint64)
    out = np.zeros(8, dtype=np.uint8)
    P = lambda a: a.ctypes.data_as(u8)
    fn = lib.blsbn254_aggregate_verify_batch

    def call(goff, n, pks=P(pk), msgs=P(ms), o=off, sigs=P(sg), tag=P(d), bm=P(out), c=ctx):
        arr = np.ascontiguousarray(np.asarray(goff, dtype=np.uint64))
        return fn(c, pks, msgs, o.ctypes.data_as(u64) if o is not None else None, arr.ctypes.data_as(u64) if len(goff) else None, sigs,
                  ctypes.c_size_t(n), tag, ctypes.c_size_t(len(dst)), bm)

    assert call([0, 2, 4], 2) == 0 and out[0] == 3
    assert call([0, 3, 1], 2) == E_ARG                                # decreasing group offsets
    assert call([0, 1 << 23], 1) == E_ARG                             # pairs + groups > 2^23: the signature's pair counts
    assert call([0, (1 << 23) - 1], 1, pks=None) == E_ARG             # (within the limit: the missing keys are the error)
    assert call([0, 2, 4], 2, pks=None) == E_ARG
    assert call([0, 2, 4], 2, msgs=None) == E_ARG
    assert call([0, 2, 4], 2, o=None) == E_ARG
    assert call([0, 2, 4], 2, sigs=None) == E_ARG
    assert call([0, 2, 4], 2, tag=None) == E_ARG
    assert call([0, 2, 4], 2, bm=None) == E_ARG
    assert call([], 2) == E_ARG                                       # no group offsets
    assert call([0, 2, 4], 2, c=None) == E_ARG
    bad_off = np.array([0, 32, 16, 64, 96], dtype=np.uint64)
    assert call([0, 2, 4], 2, o=bad_off) == E_ARG                     # decreasing message offsets
    assert call([0], 0) == 0 and call([], 0, pks=None, msgs=None, o=None, sigs=None, tag=None, bm=None) == 0
    assert lib.blsbn254_aggregate_batch_stats(ctx, None) == E_ARG
    assert lib.blsbn254_aggregate_batch_stats(None, (ctypes.c_uint64 * 4)()) == E_ARG
    assert eng.aggregate_verify_batch([], [], b"", dst) == b""
    assert eng.aggregate_verify_batch([b"", b""], [[], []], b"".join(G.sigs), dst) == b"\x00"     # empty groups only: invalid
    with pytest.raises(ValueError):
        eng.aggregate_verify_batch(G.key_sets(), [G.msgs[0]], b"".join(G.sigs), dst)
    with pytest.raises(ValueError):
        eng.aggregate_verify_batch(G.key_sets(), [G.msgs[0], G.msgs[1][:1]], b"".join(G.sigs), dst)
