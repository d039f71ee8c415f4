"""GPU tests (MI355X) of the message expander as a setting of the context (blsbn254_set_expander): the hashing kernels of
k_hash_keccak.hip against the model of tests/expander_support.py (pinned by tests/test_expander_model.py) for XMD over Keccak-256
and SHA3-256 and XOF over SHAKE-128 and SHAKE-256; every call family following the setter; the setter settling the asynchronous
verify path before it stores the new id; the resident tag dropped with it.  Expected values never come from the context under
test: points and scalars from the model, bitmaps from closed forms."""
import contextlib
import random

import numpy as np
import pytest

from oracle.pyref import bn254 as ref
from tests import expander_support as X
from tests import synth
from tests.gpu_support import eng, M  # noqa: F401 (fixtures)
from tests.helpers import b32
from tests.threshold_support import Deal

pytestmark = pytest.mark.gpu
R = synth.R
DSTS = {1: b"D", 43: b"BLS_SIG_BN254G1_XMD:KECCAK-256_SVDW_RO_NUL_", 255: b"d" * 255, 256: b"e" * 256, 300: (b"expander-tag:" * 24)[:300]}
DST = DSTS[43]
assert all(len(v) == k for k, v in DSTS.items())


@contextlib.contextmanager
def under(e, xid):
    """the engine under expander xid, back to what it was afterwards"""
    was = e.expander
    e.set_expander(xid)
    try:
        yield e
    finally:
        e.set_expander(was)


def ones(n):
    return synth.bitmap_of([True] * n)


def zeros(n):
    return bytes((n + 7) // 8)


def ragged_messages(xid, dst, n, seed):
    """the four pad-boundary lengths of this expander and tag, the empty message, 1000 bytes, then ragged lengths up to n messages:
    the lanes of one wave absorb different numbers of blocks"""
    rnd = random.Random(seed)
    msgs = X.boundary_messages(xid, dst)
    return msgs + [rnd.randbytes(rnd.randrange(0, 300)) for _ in range(n - len(msgs))]


# ================================================================ parity with the model
@pytest.mark.parametrize("dl", sorted(DSTS))
@pytest.mark.parametrize("xid", X.IDS[1:])
def test_hash_calls_equal_the_model(eng, xid, dl):
    dst = DSTS[dl]
    msgs = ragged_messages(xid, dst, 65, 100 * xid + dl)
    with under(eng, xid):
        h1, e1, sc = eng.hash_to_g1_batch(msgs, dst), eng.encode_to_g1_batch(msgs, dst), eng.hash_to_scalar_batch(msgs, dst)
        h2, e2 = eng.hash_to_g2_batch(msgs[:9], dst), eng.encode_to_g2_batch(msgs[:9], dst)
    for i, m in enumerate(msgs):
        assert h1[64 * i:64 * i + 64] == ref.g1_to_bytes(X.hash_to_g1(xid, m, dst)), ("hash_to_g1", i, len(m))
        assert e1[64 * i:64 * i + 64] == ref.g1_to_bytes(X.encode_to_g1(xid, m, dst)), ("encode_to_g1", i, len(m))
        assert sc[32 * i:32 * i + 32] == b32(X.hash_to_scalar(xid, m, dst)), ("hash_to_scalar", i, len(m))
    for i, m in enumerate(msgs[:9]):
        assert h2[128 * i:128 * i + 128] == ref.g2_to_bytes(X.hash_to_g2(xid, m, dst)), ("hash_to_g2", i, len(m))
        assert e2[128 * i:128 * i + 128] == ref.g2_to_bytes(X.encode_to_g2(xid, m, dst)), ("encode_to_g2", i, len(m))


# ================================================================ the other workspace forms, through verify
class Signed:
    """n tuples over `pool` keys (key0 ..), 32-byte messages, signed by the engine under expander xid; every bad_every-th message
    has one bit flipped afterwards, so its tuple is invalid under any expander"""
    def __init__(self, e, xid, n, pool, dst, key0=0, base=0, bad_every=0):
        self.n, self.dst = n, dst
        self.sks = [synth.sk_of(key0 + k) for k in range(pool)]
        pkp = e.sk_to_pk_batch(b"".join(map(b32, self.sks)), pool)
        self.pks = b"".join(pkp[128 * (i % pool):128 * (i % pool) + 128] for i in range(n))
        self.msgs = [synth.msg_of(base + i) for i in range(n)]
        with under(e, xid):
            self.sigs = e.sign_batch(b"".join(b32(self.sks[i % pool]) for i in range(n)), self.msgs, dst)
        self.exp = [True] * n
        for i in range(bad_every - 1, n, bad_every) if bad_every else ():
            self.msgs[i] = bytes([self.msgs[i][0] ^ 1]) + self.msgs[i][1:]
            self.exp[i] = False
        self.want = synth.bitmap_of(self.exp)

    def args(self):
        return self.pks, self.msgs, self.sigs, self.dst


def test_verify_follows_the_expander_in_every_workspace_form(eng):
    """64 + 1 tuples signed under Keccak-256: hash-to-G1 in the homogeneous form (prepared path, RLC) and in the affine form
    (exact path), each under ids 1, 0 and 2 -- SHA-3 differs from Keccak in the domain byte alone"""
    n = 65
    b = Signed(eng, X.XMD_KECCAK256, n, 8, DST, key0=7000)
    for i in (0, 31, 64):
        assert b.sigs[64 * i:64 * i + 64] == ref.g1_to_bytes(X.sign(X.XMD_KECCAK256, b.sks[i % 8], b.msgs[i], DST)), i
    bad = list(b.msgs); bad[40] = bad[40][:-1] + bytes([bad[40][-1] ^ 0x80])
    one_off = synth.bitmap_of([i != 40 for i in range(n)])
    for prepare in (True, False):
        eng.set_auto_prepare(prepare)
        try:
            for xid, want in ((X.XMD_KECCAK256, ones(n)), (X.XMD_SHA256, zeros(n)), (X.XMD_SHA3_256, zeros(n))):
                with under(eng, xid):
                    assert eng.verify_batch(*b.args()) == want, (prepare, xid)
                    assert eng.verify_batch_rlc(*b.args()) == want, (prepare, xid)
            with under(eng, X.XMD_KECCAK256):
                assert eng.verify_batch(b.pks, bad, b.sigs, DST) == one_off
                assert eng.verify_batch_rlc(b.pks, bad, b.sigs, DST) == one_off
        finally:
            eng.set_auto_prepare(True)


# ================================================================ one call of each family
def test_aggregate_verify_batch_follows_the_expander(eng):
    sizes = (1, 2, 4)
    b = Signed(eng, X.XMD_KECCAK256, sum(sizes), 7, DST, key0=7100, base=500)
    keys, msgs, aggs, lo = [], [], b"", 0
    for k in sizes:
        keys.append(b.pks[128 * lo:128 * (lo + k)]); msgs.append(b.msgs[lo:lo + k])
        aggs += eng.aggregate_sigs(b.sigs[64 * lo:64 * (lo + k)], k)
        lo += k
    with under(eng, X.XMD_KECCAK256):
        assert eng.aggregate_verify_batch(keys, msgs, aggs, DST) == ones(3)
        assert eng.aggregate_verify_batch_rlc(keys, msgs, aggs, DST) == ones(3)
    assert eng.expander == X.XMD_SHA256
    assert eng.aggregate_verify_batch(keys, msgs, aggs, DST) == zeros(3)


def test_keyset_fast_aggregate_verify_follows_the_expander(eng, M):
    nk = 33
    sks = [synth.sk_of(7200 + k) for k in range(nk)]
    pks = eng.sk_to_pk_batch(b"".join(map(b32, sks)), nk)
    sels = [[0, 5, 32], list(range(1, 33, 2))]
    rows = [np.packbits(np.array([k in s for k in range(nk)], dtype=np.uint8), bitorder="little").tobytes() for s in sels]
    msgs = [b"key set, group 0", b"key set, group 1"]
    ks = M.KeySet(eng, pks, nk)
    try:
        with under(eng, X.XMD_KECCAK256):
            sigs = eng.sign_batch(b"".join(b32(sum(sks[k] for k in s) % R) for s in sels), msgs, DST)
            assert sigs[:64] == ref.g1_to_bytes(X.sign(X.XMD_KECCAK256, sum(sks[k] for k in sels[0]) % R, msgs[0], DST))
            assert eng.keyset_fast_aggregate_verify_batch(ks, rows, msgs, sigs, DST) == ones(2)
        assert eng.keyset_fast_aggregate_verify_batch(ks, rows, msgs, sigs, DST) == zeros(2)
    finally:
        ks.close()


def test_threshold_combine_checked_follows_the_expander(eng, M):
    with under(eng, X.XMD_KECCAK256):
        d = Deal(eng, [3, 3], [2, 2], 77, DST)                     # partial signatures made under Keccak-256
        sigs, used, status = eng.threshold_combine_checked_batch(*d.args())
        assert bytes(status) == b"\0\0" and used == synth.bitmap_of([True, True, False] * 2)
        for g in range(2):
            assert sigs[64 * g:64 * g + 64] == ref.g1_to_bytes(X.sign(X.XMD_KECCAK256, d.coefs[g][0], d.msgs[g], DST)), g
    sigs0, used0, status0 = eng.threshold_combine_checked_batch(*d.args())
    assert bytes(status0) == bytes([M.ST_SHORT]) * 2 and used0 == zeros(6)


def test_proofs_of_possession_follow_the_expander(eng, M):
    n = 5
    sks = [synth.sk_of(7300 + k) for k in range(n)]
    skb = b"".join(map(b32, sks))
    pks = eng.sk_to_pk_batch(skb, n)
    pop_dst = M.POP_DST
    with under(eng, X.XMD_KECCAK256):
        proofs = eng.pop_prove_batch(skb, n)
        assert proofs[:64] == ref.g1_to_bytes(X.sign(X.XMD_KECCAK256, sks[0], pks[:128], pop_dst))
        assert eng.pop_verify_batch(pks, proofs, n) == ones(n)
        ks = M.KeySet(eng, pks, n, proofs=proofs)
        try:
            assert ks.checked() and ks.valid_bitmap() == ones(n)
        finally:
            ks.close()
    assert eng.pop_verify_batch(pks, proofs, n) == zeros(n)
    ks = M.KeySet(eng, pks, n, proofs=proofs)
    try:
        assert ks.valid_bitmap() == zeros(n)
    finally:
        ks.close()


# ================================================================ the setter settles the context
def run_dev(e, t, n, dst, bm):
    e.verify_batch_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), n, bm.data_ptr(), dst)


def test_the_setter_settles_pending_calls_under_the_old_expander(eng, M):
    """A (40 keys, Keccak-256) twice, so the context enqueues on a guess of 40 keys; B (1300 keys, more than the capacity of 1024,
    Keccak-256) is enqueued on that guess, which fails: its re-run is pending.  set_expander(0) must run it -- under Keccak-256 --
    before it stores the new id; C is signed and verified under SHA-256.  A setter that only stored the id would leave B's re-run
    to C's entry, under SHA-256, where none of B's signatures verifies.  Against a library built with such a setter the re-run
    count right behind the setter is 0 and this test fails there."""
    import torch
    n = 1300
    A = Signed(eng, X.XMD_KECCAK256, n, 40, DST, key0=7400, base=1000, bad_every=7)
    B = Signed(eng, X.XMD_KECCAK256, n, n, DST, key0=7500, base=3000, bad_every=11)
    C = Signed(eng, X.XMD_SHA256, n, 40, DST, key0=7400, base=5000, bad_every=9)
    e = M.Engine(0, expander=X.XMD_KECCAK256)
    try:
        tA, tB, tC = (synth.dev_batch(M, torch, x.pks, x.msgs, x.sigs) for x in (A, B, C))
        run_dev(e, tA, n, DST, tA[4]); e.synchronize()
        assert bytes(tA[4].cpu().numpy()) == A.want
        tA[4].fill_(0x5a); torch.cuda.synchronize()
        a0, r0 = e.async_stats()
        run_dev(e, tA, n, DST, tA[4])                                  # prepared path, enqueued on the guess
        run_dev(e, tB, n, DST, tB[4])                                  # pending; its guess fails
        assert e.async_stats()[0] == a0 + 2, "the calls were not enqueued asynchronously"
        e.set_expander(X.XMD_SHA256)
        assert e.async_stats() == (a0 + 2, r0 + 1), "the setter did not settle the pending calls"
        assert e.expander == X.XMD_SHA256
        run_dev(e, tC, n, DST, tC[4])
        e.synchronize()
        got = [bytes(t[4].cpu().numpy()) for t in (tA, tB, tC)]
        assert got[0] == A.want
        assert got[1] == B.want, "B was re-run under the new expander: popcount %d" % int(np.unpackbits(np.frombuffer(got[1], dtype=np.uint8)).sum())
        assert got[2] == C.want
        assert e.async_stats()[1] == r0 + 1
    finally:
        e.close()


# ================================================================ the resident tag
def test_sequence_of_expanders_on_one_context_with_one_oversize_tag(eng, M):
    """ids 1, 0, 4, 1 with the same 300-byte tag: what is staged for it depends on the expander, so a tag that stayed resident
    across the setter would hash under the previous expander's 32 bytes"""
    dst = DSTS[300]
    msgs = [b"", b"abc", bytes(range(200))]
    outs = []
    e = M.Engine(0)
    try:
        for xid in (1, 0, 4, 1):
            e.set_expander(xid)
            outs.append((xid, e.hash_to_g1_batch(msgs, dst), e.hash_to_scalar_batch(msgs, dst)))
    finally:
        e.close()
    for xid, g1, sc in outs:
        f = M.Engine(0, expander=xid)
        try:
            assert f.expander == xid
            assert (g1, sc) == (f.hash_to_g1_batch(msgs, dst), f.hash_to_scalar_batch(msgs, dst)), xid
        finally:
            f.close()
        assert g1 == b"".join(ref.g1_to_bytes(X.hash_to_g1(xid, m, dst)) for m in msgs), xid
    assert outs[0][1:] == outs[3][1:] and outs[0][1] != outs[1][1] != outs[2][1]


def test_a_bad_id_is_refused_and_changes_nothing(eng, M):
    msgs = [b"still Keccak"]
    with under(eng, X.XMD_KECCAK256):
        before = eng.hash_to_g1_batch(msgs, DST)
        for bad in (5, -1, 99):
            with pytest.raises(M.Bn254Error) as err:
                eng.set_expander(bad)
            assert err.value.code == -1
            assert eng.expander == X.XMD_KECCAK256
        assert eng.hash_to_g1_batch(msgs, DST) == before == ref.g1_to_bytes(X.hash_to_g1(X.XMD_KECCAK256, msgs[0], DST))
