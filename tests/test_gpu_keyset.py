"""GPU tests (MI355X) of the sums over a registered key set selected by bitmaps (blsbn254_keyset_*): edge sets against the
oracle and against the parent's entry points on the gathered key lists, workgroup and launch boundaries, the committee shape,
several handles and other call families on one context, the argument errors.  Expected values never come from the calls under
test: the oracle, closed forms, or blsbn254_fast_aggregate_verify_batch / blsbn254_aggregate_pks on the gathered lists."""
import ctypes
import random

import numpy as np
import pytest

from tests import synth
from tests.gpu_support import eng, M
from tests.helpers import b32, bits_of, IDENT1, IDENT2, row_of
from tests.keyset_support import Committee, edge_rows, sign_rows

pytestmark = pytest.mark.gpu
R = synth.R
E_ARG = -1
u8 = ctypes.POINTER(ctypes.c_uint8)
u64 = ctypes.POINTER(ctypes.c_uint64)


@pytest.mark.parametrize("n", [1, 33, 70, 513])
def test_edge_sets(eng, oracle, M, n):
    dst = M.DEFAULT_DST
    rnd = random.Random(77 + n)
    com = Committee(eng, n, n)
    rows, named = edge_rows(com, rnd)
    G = len(rows)
    msgs = [b"keyset edge %d/%d" % (n, g) for g in range(G)]
    sigs = sign_rows(eng, com, rows, msgs, dst)
    msgs[named["tampered"]] += b"!"
    sigs[64 * named["ident_sig"]:64 * named["ident_sig"] + 64] = IDENT1
    sigs = bytes(sigs)
    s0 = eng.keyset_stats()
    ks = M.KeySet(eng, com.pks, n)
    try:
        assert ks.count() == n
        sel = [row_of(r, n) for r in rows]
        out, status = eng.keyset_sum_batch(ks, sel)
        got = eng.keyset_fast_aggregate_verify_batch(ks, b"".join(sel), msgs, sigs, dst)
        valid = ks.valid_bitmap()
    finally:
        ks.close()
    s1 = eng.keyset_stats()
    # sums
    assert list(status) == [0 if r & com.bad else 1 for r in rows]
    for g, r in enumerate(rows):
        want = oracle.aggregate_pks(com.gather(r), len(r)) if status[g] else IDENT2
        assert out[128 * g:128 * g + 128] == want, (n, g)
    if com.at:
        assert status[named["flipped_with_bad"]] == 0 and 2 * len(rows[named["flipped_with_bad"]]) > n
        assert out[128 * named["p_negp"]:128 * named["p_negp"] + 128] == IDENT2
    # verification bits
    lists = [com.gather(r) for r in rows]
    want_bits = [oracle.fast_aggregate_verify(lists[g], len(r), msgs[g], sigs[64 * g:64 * g + 64], dst) for g, r in enumerate(rows)]
    assert got == synth.bitmap_of(want_bits)
    assert got == eng.fast_aggregate_verify_batch(lists, msgs, sigs, dst)
    expect_true = [g for g, r in enumerate(rows) if r and not (r & com.unsignable) and g not in (named["tampered"], named["ident_sig"])
                   and com.group_sk(r) == sum(com.sk[i] for i in r) % R]
    assert all(want_bits[g] for g in expect_true) and len(expect_true) >= (1 if n == 1 else 8)
    for name in ("tampered", "ident_sig") + (("p_negp", "nonsub", "flipped_with_bad") if com.at else ()):
        assert not want_bits[named[name]], name
    if com.at:
        assert want_bits[named["dup"]] and want_bits[named["ident"]] and want_bits[named["boundary"]]
        assert 2 * len(rows[named["boundary"]]) > n >= 2 * (len(rows[named["boundary"]]) - 1)
    # KeyValidate per registered key
    chk = bits_of(oracle.g2_check_batch(com.pks, n), n)
    if com.at:
        assert chk[com.at["ident"]]
        chk[com.at["ident"]] = False
    assert valid == synth.bitmap_of(chk)
    # counters: both calls served every row
    flips = sum(1 for r in rows if 2 * len(r) > n)
    assert s1["groups"] - s0["groups"] == 2 * G and s1["complement_groups"] - s0["complement_groups"] == 2 * flips
    assert s1["key_sets"] - s0["key_sets"] == 1 and s1["launches"] - s0["launches"] == 2


def test_workgroup_and_launch_boundaries(eng, M, monkeypatch):
    dst = M.DEFAULT_DST
    n, G = 70, 257                                                      # 3 words; one group past the 256-group workgroup
    rnd = random.Random(5)
    com = Committee(eng, n, 2)
    good = [i for i in range(n) if i not in com.unsignable]
    rows = [{i for i in (good if g % 5 else range(n)) if rnd.random() < (0.3, 0.6, 0.95)[g % 3]} for g in range(G)]
    rows[255], rows[256] = set(good), {good[0]}
    msgs = [synth.msg_of(70000 + g) for g in range(G)]
    sigs = sign_rows(eng, com, rows, msgs, dst)
    for g in range(0, G, 9):
        msgs[g] = bytes([msgs[g][0] ^ 1]) + msgs[g][1:]
    sigs = bytes(sigs)
    sel = b"".join(row_of(r, n) for r in rows)
    want = eng.fast_aggregate_verify_batch([com.gather(r) for r in rows], msgs, sigs, dst)
    want_bits = bits_of(want, G)
    assert not any(want_bits[g] for g in range(0, G, 9)) and sum(want_bits) > G // 2
    results = []
    for chunk in (None, "304"):                                         # 304 / 3 words -> launches of 96 groups: 96 + 96 + 65
        with monkeypatch.context() as mp:
            if chunk:
                mp.setenv("BLSBN254_CHUNK_LANES", chunk)
            e = M.Engine(0)
            try:
                ks = M.KeySet(e, com.pks, n)
                results.append((e.keyset_fast_aggregate_verify_batch(ks, sel, msgs, sigs, dst), e.keyset_sum_batch(ks, sel)))
                assert e.keyset_stats()["launches"] == (6 if chunk else 2)
                ks.close()
            finally:
                e.close()
    assert results[0] == results[1] and results[0][0] == want
    out, status = results[0][1]
    assert list(status) == [0 if r & com.bad else 1 for r in rows]
    for g in (0, 1, 95, 96, 191, 192, 255, 256):
        if status[g]:
            assert out[128 * g:128 * g + 128] == eng.aggregate_pks(com.gather(rows[g]), len(rows[g])), g


def test_committee_shape(eng, oracle, M):
    """1024 keys, 512 aggregates at about 2/3 participation: every row goes through the complement"""
    dst = M.DEFAULT_DST
    n, G = 1024, 512
    rnd = random.Random(11)
    com = Committee(eng, n, 3, special=False)
    rows = [{i for i in range(n) if rnd.random() < 2 / 3} for _ in range(G)]
    assert all(2 * len(r) > n for r in rows)
    msgs = [synth.msg_of(90000 + g) for g in range(G)]
    sigs = bytes(sign_rows(eng, com, rows, msgs, dst))
    exp = []
    for g in range(G):
        ok = g % 7 != 6
        if not ok:
            msgs[g] = bytes([msgs[g][0] ^ 1]) + msgs[g][1:]
        exp.append(ok)
    ks = M.KeySet(eng, com.pks, n)
    try:
        s0 = eng.keyset_stats()
        got = eng.keyset_fast_aggregate_verify_batch(ks, [row_of(r, n) for r in rows], msgs, sigs, dst)
        s1 = eng.keyset_stats()
    finally:
        ks.close()
    lists = [com.gather(r) for r in rows]
    assert got == synth.bitmap_of(exp)
    assert got == eng.fast_aggregate_verify_batch(lists, msgs, sigs, dst)
    for g in (0, 6, G - 1):
        assert oracle.fast_aggregate_verify(lists[g], len(rows[g]), msgs[g], sigs[64 * g:64 * g + 64], dst) is exp[g]
    assert s1["complement_groups"] - s0["complement_groups"] == G and s1["groups"] - s0["groups"] == G


def test_two_key_sets_and_other_calls_on_one_context(eng, oracle, M):
    import torch
    dst = M.DEFAULT_DST
    dst2 = dst[:-1] + bytes([dst[-1] ^ 1])                              # another tag of the same length
    rnd = random.Random(21)
    coms = [Committee(eng, 70, 4), Committee(eng, 200, 5, special=False)]
    calls = []
    for c, tag in zip(coms, (dst, dst2)):
        good = [i for i in range(c.n) if i not in c.unsignable]
        rows = [{i for i in good if rnd.random() < (0.2, 0.8)[g & 1]} | {good[0]} for g in range(40)]
        msgs = [b"two sets %d/%d" % (c.n, g) for g in range(40)]
        sigs = bytes(sign_rows(eng, c, rows, msgs, tag))
        msgs[3] += b"?"
        calls.append((b"".join(row_of(r, c.n) for r in rows), msgs, sigs, tag, [c.gather(r) for r in rows]))
    vb = synth.make_batch_gpu(eng, oracle, 600, dst, pool=40, invalid_every=7, spot=4)
    scal = b"".join(b32(rnd.randrange(R)) for _ in range(70))
    msm_pts = b"".join(coms[1].keys[:70])

    def fresh(f):
        e = M.Engine(0)
        try:
            return f(e)
        finally:
            e.close()

    def ks_call(e, k, which, fav=True):
        sel, msgs, sigs, tag, _ = calls[which]
        return e.keyset_fast_aggregate_verify_batch(k, sel, msgs, sigs, tag) if fav else e.keyset_sum_batch(k, sel)

    def alone(which, fav=True):
        def f(e):
            k = M.KeySet(e, coms[which].pks, coms[which].n)
            try:
                return ks_call(e, k, which, fav)
            finally:
                k.close()
        return fresh(f)

    want = {(w, fav): alone(w, fav) for w in (0, 1) for fav in (True, False)}
    for w in (0, 1):                                                    # ... which are what the parent's call gives on the lists
        sel, msgs, sigs, tag, lists = calls[w]
        assert want[(w, True)] == eng.fast_aggregate_verify_batch(lists, msgs, sigs, tag)
        assert sum(bits_of(want[(w, True)], 40)) == 39
    want_fav = fresh(lambda e: e.fast_aggregate_verify_batch(calls[0][4], calls[0][1], calls[0][2], calls[0][3]))
    want_agg = fresh(lambda e: e.aggregate_pks(msm_pts, 70))
    want_msm = fresh(lambda e: e.g2_msm(msm_pts, scal, 70))
    t = synth.dev_batch(M, torch, vb[0], vb[1], vb[2])
    e = M.Engine(0)
    try:
        k0, k1 = M.KeySet(e, coms[0].pks, 70), M.KeySet(e, coms[1].pks, 200)
        assert ks_call(e, k0, 0) == want[(0, True)]
        assert ks_call(e, k1, 1) == want[(1, True)]                     # the other set, the other tag
        assert ks_call(e, k0, 0) == want[(0, True)]                     # ... and the first tag again
        e.verify_batch_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), 600, t[4].data_ptr(), dst)     # left pending
        assert ks_call(e, k1, 1, fav=False) == want[(1, False)]
        e.synchronize()
        assert t[4].cpu().numpy().tobytes() == synth.bitmap_of(vb[3])
        assert e.fast_aggregate_verify_batch(calls[0][4], calls[0][1], calls[0][2], calls[0][3]) == want_fav
        assert ks_call(e, k0, 0, fav=False) == want[(0, False)]
        assert e.aggregate_pks(msm_pts, 70) == want_agg
        assert ks_call(e, k1, 1) == want[(1, True)]
        assert e.g2_msm(msm_pts, scal, 70) == want_msm
        assert ks_call(e, k0, 0) == want[(0, True)]
        k0.close()                                                      # one set destroyed: the other still answers
        assert ks_call(e, k1, 1) == want[(1, True)] and ks_call(e, k1, 1, fav=False) == want[(1, False)]
        assert k1.valid_bitmap() == synth.bitmap_of([True] * 200)
        assert e.keyset_stats()["key_sets"] == 2
        k1.close()
    finally:
        e.close()


def test_argument_errors(eng, M):
    lib, ctx = eng._lib, eng._ctx
    dst = b"TEST"
    n = 13                                                              # rows of 2 bytes, 3 padding bits
    com = Committee(eng, n, 6)
    rows = [{0, 1, 12}, set(range(n)), {5}]
    msgs = [b"a", b"bc", b"def"]
    sigs = bytes(sign_rows(eng, com, rows, msgs, dst))
    sel = np.frombuffer(b"".join(row_of(r, n) for r in rows), dtype=np.uint8).copy()
    pks = np.frombuffer(com.pks, dtype=np.uint8)
    data = np.frombuffer(b"".join(msgs), dtype=np.uint8)
    off = np.array([0, 1, 3, 6], dtype=np.uint64)
    sg = np.frombuffer(sigs, dtype=np.uint8)
    out = np.zeros(128 * 3, dtype=np.uint8); st = np.zeros(3, dtype=np.uint8); bm = np.zeros(1, dtype=np.uint8)
    P = lambda a: a.ctypes.data_as(u8)

    def create(c=ctx, p=P(pks), k=n, out_h=True):
        h = ctypes.c_void_p()
        return lib.blsbn254_keyset_create(c, p, ctypes.c_size_t(k), ctypes.byref(h) if out_h else None), h

    rc, h = create()
    assert rc == 0 and lib.blsbn254_keyset_count(h) == n
    assert create(c=None)[0] == E_ARG and create(p=None)[0] == E_ARG and create(out_h=False)[0] == E_ARG
    rc0, h0 = create(k=0)
    assert rc0 == E_ARG and not h0.value
    assert create(k=65537)[0] == E_ARG
    assert lib.blsbn254_keyset_count(None) == 0
    lib.blsbn254_keyset_destroy(None)

    def sums(c=ctx, k=h, s=P(sel), g=3, o=P(out), t=P(st)):
        return lib.blsbn254_keyset_sum_batch(c, k, s, ctypes.c_size_t(g), o, t)

    def fav(c=ctx, k=h, s=P(sel), m=P(data), of=off.ctypes.data_as(u64), sig=P(sg), g=3, d=dst, dl=4, b=P(bm)):
        return lib.blsbn254_keyset_fast_aggregate_verify_batch(c, k, s, m, of, sig, ctypes.c_size_t(g), d, ctypes.c_size_t(dl), b)

    assert sums() == 0 and st.tobytes() == b"\x01" * 3 and fav() == 0 and bm[0] == 7
    for name in ("c", "k", "s", "o", "t"):
        assert sums(**{name: None}) == E_ARG, name
    for name in ("c", "k", "s", "of", "sig", "d", "b"):
        assert fav(**{name: None}) == E_ARG, name
    assert sums(g=0) == 0 and fav(g=0) == 0 and sums(g=0, s=None, o=None, t=None) == 0
    e2 = M.Engine(0)                                                    # a key set that belongs to another context
    try:
        assert sums(c=e2._ctx) == E_ARG and fav(c=e2._ctx) == E_ARG
        assert lib.blsbn254_keyset_valid(e2._ctx, h, P(bm)) == E_ARG
    finally:
        e2.close()
    assert lib.blsbn254_keyset_valid(ctx, h, None) == E_ARG and lib.blsbn254_keyset_valid(ctx, None, P(bm)) == E_ARG
    for g, bit in ((0, 5), (2, 7), (1, 6)):                             # a padding bit (index >= 13) in a row's last byte
        sel[2 * g + 1] ^= 1 << bit
        assert sums() == E_ARG and fav() == E_ARG and b"row %d" % g in lib.blsbn254_last_error(ctx)
        sel[2 * g + 1] ^= 1 << bit
    assert lib.blsbn254_keyset_stats(ctx, None) == E_ARG and lib.blsbn254_keyset_stats(None, (ctypes.c_uint64 * 4)()) == E_ARG
    st[:] = 0x5a; bm[:] = 0
    assert sums() == 0 and st.tobytes() == b"\x01" * 3 and fav() == 0 and bm[0] == 7      # after the errors, the context still serves
    assert out.tobytes()[128 * 2:] == com.keys[5]
    lib.blsbn254_keyset_destroy(h)
    ks = M.KeySet(eng, com.pks, n)
    try:
        with pytest.raises(ValueError):
            eng.keyset_sum_batch(ks, [b"\x00"])
        with pytest.raises(ValueError):
            eng.keyset_fast_aggregate_verify_batch(ks, [bytes(2)], [], b"", dst)
        with pytest.raises(M.Bn254Error):
            eng.keyset_sum_batch(ks, [b"\x00\x20"])
        assert eng.keyset_sum_batch(ks, []) == (b"", b"")
    finally:
        ks.close()
