"""GPU tests (MI355X) of the map to G1 as a setting of the context (blsbn254_set_g1_map): the kernels of k_hash_tai.hip against
the model of tests/g1_map_support.py (pinned by tests/test_g1_map_model.py) on launches that mix short and long searches in one
wave; every workspace mode; every call family following the setter and the proofs of possession not following it; the setter
settling the asynchronous verify path before it stores the new id.  Expected values never come from the context under test:
points from the model, signatures through the oracle's G1 multiplication, bitmaps from closed forms.  The tag is ignored under
the try-and-increment ids, so the calls pass one that no other test uses."""
import contextlib
import random

import numpy as np
import pytest

from oracle import oracle as O
from tests import expander_support as X
from tests import g1_map_support as G
from tests import synth
from tests.gpu_support import eng, M  # noqa: F401 (fixtures)
from tests.helpers import b32
from tests.threshold_support import Deal

pytestmark = pytest.mark.gpu
R = synth.R
DST = b"a tag the try-and-increment map never reads"


@contextlib.contextmanager
def under(e, map_id, xid=None):
    """the engine under the map (and expander), back to what it was afterwards"""
    was, wasx = e.get_g1_map(), e.expander
    e.set_g1_map(map_id)
    if xid is not None:
        e.set_expander(xid)
    try:
        yield e
    finally:
        e.set_g1_map(was)
        e.set_expander(wasx)


def ones(n):
    return synth.bitmap_of([True] * n)


def zeros(n):
    return bytes((n + 7) // 8)


def model_points(map_id, xid, msgs):
    return b"".join(G.hash_bytes(map_id, xid, m) for m in msgs)


def model_sign(map_id, xid, sk, msg):
    """[sk] (model point), the multiplication by the oracle"""
    return O.g1_mul(G.hash_bytes(map_id, xid, msg), sk % R)


# ================================================================ 1. parity with the model, searches of mixed length in one wave
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_hash_to_g1_under_tai_digest_equals_the_model(eng, n):
    """fails on a library without the setting: the engine has no blsbn254_set_g1_map to call"""
    msgs = G.mixed_wave(n)
    with under(eng, G.TAI_DIGEST):
        got = eng.hash_to_g1_batch(msgs, DST)
    for i, m in enumerate(msgs):
        assert got[64 * i:64 * i + 64] == G.hash_bytes(G.TAI_DIGEST, 0, m), (i, G.run_of(G.x0_of(G.TAI_DIGEST, 0, m)))


def test_waves_of_equal_and_of_long_searches(eng):
    short, long_ = G.digests_with_run(0, 64), G.digests_with_run(3, 64, at_least=True)
    with under(eng, G.TAI_DIGEST):
        assert eng.hash_to_g1_batch(short, DST) == model_points(G.TAI_DIGEST, 0, short)
        assert eng.hash_to_g1_batch(long_, DST) == model_points(G.TAI_DIGEST, 0, long_)
        odd = G.ODD_LENGTHS + G.EDGE_DIGESTS                   # other lengths reduce as one big-endian integer
        assert eng.hash_to_g1_batch(odd, DST) == model_points(G.TAI_DIGEST, 0, odd)


# ================================================================ 2. the plain hashes
@pytest.mark.parametrize("xid", X.IDS)
def test_hash_to_g1_under_tai_hash_equals_the_model(eng, xid):
    rnd = random.Random(650 + xid)
    msgs = [b""] + [rnd.randbytes(rnd.randrange(0, 201)) for _ in range(63)] + [rnd.randbytes(200)]
    assert len(msgs) == 65
    with under(eng, G.TAI_HASH, xid):
        got = eng.hash_to_g1_batch(msgs, DST)
        again = eng.hash_to_g1_batch(msgs, b"another tag")
    assert got == again, "the tag is read"
    for i, m in enumerate(msgs):
        assert got[64 * i:64 * i + 64] == G.hash_bytes(G.TAI_HASH, xid, m), (i, len(m))


# ================================================================ signed batches
class Signed:
    """n tuples over `pool` keys, 32-byte digests with mixed runs as messages, signed by the engine under (map_id, xid); the
    tuples of `bad` have one bit of their message's FIRST byte flipped afterwards (the last bit would only move x0 by one, to a
    neighbour that may well search to the same point)"""
    def __init__(self, e, map_id, n, pool, key0, seed=0, xid=None, bad=(), msgs=None):
        self.n = n
        self.sks = [synth.sk_of(key0 + k) for k in range(pool)]
        pkp = e.sk_to_pk_batch(b"".join(map(b32, self.sks)), pool)
        self.key = [i % pool for i in range(n)]
        self.pks = b"".join(pkp[128 * k:128 * k + 128] for k in self.key)
        self.msgs = list(msgs) if msgs is not None else G.mixed_wave(n, seed)
        with under(e, map_id, xid):
            self.sigs = e.sign_batch(b"".join(b32(self.sks[k]) for k in self.key), self.msgs, DST)
        self.exp = [i not in bad for i in range(n)]
        for i in bad:
            self.msgs[i] = bytes([self.msgs[i][0] ^ 1]) + self.msgs[i][1:]
        self.want = synth.bitmap_of(self.exp)

    def args(self):
        return self.pks, self.msgs, self.sigs, DST


@pytest.fixture(scope="module")
def batch(eng):
    """130 tuples over 8 keys under TAI_DIGEST, three of them spoiled; shared, never changed"""
    return Signed(eng, G.TAI_DIGEST, 130, 8, 8100, bad=(3, 64, 129))


# ================================================================ 3. every workspace mode;  4. sign and the call families
def test_sign_batch_is_the_scalar_multiple_of_the_model_point(eng, batch):
    good = Signed(eng, G.TAI_DIGEST, 65, 8, 8100, seed=1)
    for i in range(65):
        assert good.sigs[64 * i:64 * i + 64] == model_sign(G.TAI_DIGEST, 0, good.sks[good.key[i]], good.msgs[i]), i
    with under(eng, G.TAI_HASH, X.XMD_KECCAK256):
        s = eng.sign_batch(b32(good.sks[0]) + b32(good.sks[1]), [b"keccak", b""], DST)
    assert s == model_sign(G.TAI_HASH, 1, good.sks[0], b"keccak") + model_sign(G.TAI_HASH, 1, good.sks[1], b"")


def test_verify_in_every_workspace_mode(eng, M, batch):
    """mode 0: the exact path of verify_batch; mode 3: its prepared path, verify_batch_rlc and verify_batch_prepared; mode 1 is
    hash_to_g1_batch above.  A signature made under one map fails under the other, both ways"""
    b = batch
    svdw = Signed(eng, G.SVDW, 65, 8, 8100)
    for prepare in (True, False):
        eng.set_auto_prepare(prepare)
        try:
            with under(eng, G.TAI_DIGEST):
                assert eng.verify_batch(*b.args()) == b.want, prepare
                assert eng.verify_batch_rlc(*b.args()) == b.want, prepare
                assert eng.verify_batch(*svdw.args()) == zeros(65), prepare
            assert eng.verify_batch(*b.args()) == zeros(b.n), prepare
            assert eng.verify_batch(*svdw.args()) == ones(65), prepare
        finally:
            eng.set_auto_prepare(True)
    pkp = eng.sk_to_pk_batch(b"".join(map(b32, b.sks)), 8)
    keys = eng.g2_prepare_batch(pkp, 8)
    try:
        with under(eng, G.TAI_DIGEST):
            assert eng.verify_batch_prepared(keys, b.key, b.msgs, b.sigs, DST) == b.want
            cp, cs = eng.g2_compress_batch(b.pks, b.n), eng.g1_compress_batch(b.sigs, b.n)
            assert eng.verify_batch_compressed(cp, b.msgs, cs, DST) == b.want
        assert eng.verify_batch_prepared(keys, b.key, b.msgs, b.sigs, DST) == zeros(b.n)
    finally:
        keys.close()


def test_aggregate_family_follows_the_map(eng, batch):
    b = Signed(eng, G.TAI_DIGEST, 65, 7, 8200, seed=2)
    sizes = (1, 2, 4, 13, 45)
    keys, msgs, aggs, lo = [], [], b"", 0
    for k in sizes:
        keys.append(b.pks[128 * lo:128 * (lo + k)]); msgs.append(b.msgs[lo:lo + k])
        aggs += eng.aggregate_sigs(b.sigs[64 * lo:64 * (lo + k)], k)
        lo += k
    spoiled = [list(m) for m in msgs]
    spoiled[3][5] = bytes([spoiled[3][5][0] ^ 1]) + spoiled[3][5][1:]
    want = synth.bitmap_of([g != 3 for g in range(5)])
    with under(eng, G.TAI_DIGEST):
        assert eng.aggregate_verify(keys[4], msgs[4], aggs[256:320], DST) is True
        assert eng.aggregate_verify(keys[3], spoiled[3], aggs[192:256], DST) is False
        assert eng.aggregate_verify_batch(keys, msgs, aggs, DST) == ones(5)
        assert eng.aggregate_verify_batch(keys, spoiled, aggs, DST) == want
        assert eng.aggregate_verify_batch_rlc(keys, msgs, aggs, DST) == ones(5)
        assert eng.aggregate_verify_batch_rlc(keys, spoiled, aggs, DST) == want
    assert eng.aggregate_verify(keys[4], msgs[4], aggs[256:320], DST) is False
    assert eng.aggregate_verify_batch(keys, msgs, aggs, DST) == zeros(5)


def test_fast_aggregate_and_key_set_calls_follow_the_map(eng, M):
    nk = 33
    sks = [synth.sk_of(8300 + k) for k in range(nk)]
    pks = eng.sk_to_pk_batch(b"".join(map(b32, sks)), nk)
    sels = [[0, 5, 32], list(range(1, 33, 2)), [7], list(range(nk))]
    rows = [np.packbits(np.array([k in s for k in range(nk)], dtype=np.uint8), bitorder="little").tobytes() for s in sels]
    msgs = G.digests_with_run(12, 1, at_least=True) + G.digests_with_run(0, 1) + G.digests_with_run(5, 1) + [G.EDGE_DIGESTS[3]]
    wrong = list(msgs); wrong[2] = G.digests_with_run(5, 2)[1]
    want = synth.bitmap_of([True, True, False, True])
    ks = M.KeySet(eng, pks, nk)
    try:
        with under(eng, G.TAI_DIGEST):
            sigs = eng.sign_batch(b"".join(b32(sum(sks[k] for k in s) % R) for s in sels), msgs, DST)
            assert sigs[:64] == model_sign(G.TAI_DIGEST, 0, sum(sks[k] for k in sels[0]) % R, msgs[0])
            sets = [b"".join(pks[128 * k:128 * k + 128] for k in s) for s in sels]
            assert eng.fast_aggregate_verify_batch(sets, msgs, sigs, DST) == ones(4)
            assert eng.fast_aggregate_verify_batch(sets, wrong, sigs, DST) == want
            assert eng.keyset_fast_aggregate_verify_batch(ks, rows, msgs, sigs, DST) == ones(4)
            assert eng.keyset_fast_aggregate_verify_batch(ks, rows, wrong, sigs, DST) == want
            # the collecting node: group 0 gets the three signatures of its signers, one of them over another digest
            singles = eng.sign_batch(b"".join(b32(sks[k]) for k in sels[0]), [msgs[0], msgs[0], wrong[2]], DST)
            entries = [{k: singles[64 * j:64 * j + 64] for j, k in enumerate(sels[0])}]
            out, orow, status = eng.keyset_aggregate_checked_batch(ks, entries, [msgs[0]], DST)
            assert bytes(status) == b"\0" and orow == np.packbits(np.array([k in (0, 5) for k in range(nk)], dtype=np.uint8), bitorder="little").tobytes()
            assert out == model_sign(G.TAI_DIGEST, 0, (sks[0] + sks[5]) % R, msgs[0])
        assert eng.fast_aggregate_verify_batch(sets, msgs, sigs, DST) == zeros(4)
        assert eng.keyset_fast_aggregate_verify_batch(ks, rows, msgs, sigs, DST) == zeros(4)
    finally:
        ks.close()


def test_threshold_combine_checked_follows_the_map(eng, M):
    with under(eng, G.TAI_HASH, X.XMD_KECCAK256):
        d = Deal(eng, [3, 3], [2, 2], 78, DST)                     # partial signatures made under the map
        sigs, used, status = eng.threshold_combine_checked_batch(*d.args())
        assert bytes(status) == b"\0\0" and used == synth.bitmap_of([True, True, False] * 2)
        for g in range(2):
            assert sigs[64 * g:64 * g + 64] == model_sign(G.TAI_HASH, 1, d.coefs[g][0], d.msgs[g]), g
    sigs0, used0, status0 = eng.threshold_combine_checked_batch(*d.args())
    assert bytes(status0) == bytes([M.ST_SHORT]) * 2 and used0 == zeros(6)


# ================================================================ 5. what does not follow the map
def test_proofs_encode_and_the_other_hashes_keep_the_rfc_map(eng, M):
    n = 5
    sks = [synth.sk_of(8400 + k) for k in range(n)]
    skb = b"".join(map(b32, sks))
    pks = eng.sk_to_pk_batch(skb, n)
    msgs = [b"", b"abc", bytes(range(100))]
    dst = M.DEFAULT_DST

    def calls(e):
        proofs = e.pop_prove_batch(skb, n)
        ks = M.KeySet(e, pks, n, proofs=proofs)
        try:
            valid = (ks.checked(), ks.valid_bitmap())
        finally:
            ks.close()
        return (proofs, e.pop_verify_batch(pks, proofs, n), valid, e.encode_to_g1_batch(msgs, dst), e.hash_to_g2_batch(msgs, dst),
                e.hash_to_scalar_batch(msgs, dst))

    want = calls(eng)
    assert want[1] == ones(n) and want[2] == (True, ones(n))
    for map_id in (G.TAI_DIGEST, G.TAI_HASH):
        with under(eng, map_id):
            assert calls(eng) == want, map_id
            assert eng.get_g1_map() == map_id, "a proof call left the map changed"
            assert eng.hash_to_g1_batch(msgs, dst) == model_points(map_id, 0, msgs)


# ================================================================ 6. sequences on one context
def test_sequence_of_maps_on_one_context(eng, M):
    msgs = G.mixed_wave(65, 2)
    outs = []
    e = M.Engine(0)
    try:
        for map_id in (1, 0, 2, 1):
            e.set_g1_map(map_id)
            outs.append((map_id, e.hash_to_g1_batch(msgs, M.DEFAULT_DST)))
    finally:
        e.close()
    for map_id, got in outs:
        f = M.Engine(0)
        try:
            f.set_g1_map(map_id)
            assert f.get_g1_map() == map_id and got == f.hash_to_g1_batch(msgs, M.DEFAULT_DST), map_id
        finally:
            f.close()
        if map_id:
            assert got == model_points(map_id, 0, msgs)
    assert outs[0][1] == outs[3][1] and len({o[1] for o in outs}) == 3
    assert outs[1][1] == O.hash_to_g1_batch(msgs, M.DEFAULT_DST)


# ================================================================ 7. the setter settles the context
def run_dev(e, t, n, bm):
    e.verify_batch_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), n, bm.data_ptr(), DST)


def test_the_setter_settles_pending_calls_under_the_old_map(eng, M):
    """As tests/test_gpu_expanders.py does for the expander.  A (40 keys, TAI_DIGEST) twice, so the context enqueues on a guess of
    40 keys; B (1300 keys, more than the guessed capacity) is enqueued on that guess, which fails: its re-run is pending.
    set_g1_map(SVDW) must run it -- under TAI_DIGEST -- before it stores the new id; C is signed and verified under SVDW.  A setter
    that only stored the id would leave B's re-run to C's entry, under SVDW, where none of B's signatures verifies: the re-run
    count right behind the setter would be 0."""
    import torch
    n = 1300
    bad = lambda step: tuple(range(step - 1, n, step))   # noqa: E731
    digests = lambda base: [synth.msg_of(base + i) for i in range(n)]   # noqa: E731 (32 bytes each: searches of every length)
    A = Signed(eng, G.TAI_DIGEST, n, 40, 8500, bad=bad(7), msgs=digests(11000))
    B = Signed(eng, G.TAI_DIGEST, n, n, 8600, bad=bad(11), msgs=digests(13000))
    C = Signed(eng, G.SVDW, n, 40, 8500, bad=bad(9), msgs=digests(15000))
    e = M.Engine(0)
    try:
        e.set_g1_map(G.TAI_DIGEST)
        tA, tB, tC = (synth.dev_batch(M, torch, x.pks, x.msgs, x.sigs) for x in (A, B, C))
        run_dev(e, tA, n, tA[4]); e.synchronize()
        assert bytes(tA[4].cpu().numpy()) == A.want
        tA[4].fill_(0x5a); torch.cuda.synchronize()
        a0, r0 = e.async_stats()
        run_dev(e, tA, n, tA[4])                                       # prepared path, enqueued on the guess
        run_dev(e, tB, n, tB[4])                                       # pending; its guess fails
        assert e.async_stats()[0] == a0 + 2, "the calls were not enqueued asynchronously"
        e.set_g1_map(G.SVDW)
        assert e.async_stats() == (a0 + 2, r0 + 1), "the setter did not settle the pending calls"
        assert e.get_g1_map() == G.SVDW
        run_dev(e, tC, n, tC[4])
        e.synchronize()
        got = [bytes(t[4].cpu().numpy()) for t in (tA, tB, tC)]
        assert got[0] == A.want
        assert got[1] == B.want, "B was re-run under the new map: popcount %d" % int(np.unpackbits(np.frombuffer(got[1], dtype=np.uint8)).sum())
        assert got[2] == C.want
        assert e.async_stats()[1] == r0 + 1
    finally:
        e.close()


# ================================================================ 8. a refused id
def test_a_bad_id_is_refused_and_changes_nothing(eng, M):
    msgs = G.digests_with_run(2, 1)
    with under(eng, G.TAI_DIGEST):
        before = eng.hash_to_g1_batch(msgs, DST)
        for bad in (3, -1, 99):
            with pytest.raises(M.Bn254Error) as err:
                eng.set_g1_map(bad)
            assert err.value.code == -1
            assert eng.get_g1_map() == G.TAI_DIGEST
        assert eng.hash_to_g1_batch(msgs, DST) == before == model_points(G.TAI_DIGEST, 0, msgs)
    assert eng.get_g1_map() == G.SVDW
