"""GPU tests (MI355X) of the registration of a key set WITH proofs of possession (blsbn254_keyset_create_checked): a key whose
proof fails is a bad key of the handle in every respect.  Expected values never come from the handle under test: the validity
bits are those of a plain handle ANDed with blsbn254_pop_verify_batch (and the oracle's verification at n = 33), and every call
on the checked handle is compared with the same call on a PLAIN handle made of the key list in which each key with a failed
proof is replaced by an encoding that does not decode."""
import random

import pytest

from tests import synth
from tests.gpu_support import eng, M
from tests.helpers import b32, bits_of, IDENT1, IDENT2, row_of
from tests.keyset_support import Committee, edge_rows, sign_rows

pytestmark = pytest.mark.gpu
UNDEC2 = b"\xff" * 128


def proofs_of(eng, com, seed):
    """a true proof for every key whose secret key is known (P and -P, the duplicate); for the others the proof of the key the
    committee first had at that index, which cannot hold for the key that replaced it"""
    first = [synth.sk_of(1000 * seed + k) for k in range(com.n)]
    sks = [com.sk[i] if com.sk[i] else first[i] for i in range(com.n)]
    p = eng.pop_prove_batch(b"".join(map(b32, sks)), com.n)
    return [p[64 * i:64 * i + 64] for i in range(com.n)]


def tamper(com, proofs):
    """-> {name: index} of the proofs spoilt: another key's proof, a flipped bit, the identity, bytes that do not decode"""
    plain = [i for i in range(com.n) if i not in com.at.values()]
    if com.n == 1:
        flip = bytearray(proofs[0]); flip[40] ^= 4
        proofs[0] = bytes(flip)
        return {"flip": 0}
    t = {"other": plain[2], "flip": plain[4], "ident": plain[6], "undec": plain[8]}
    proofs[t["other"]] = proofs[plain[10]]
    flip = bytearray(proofs[t["flip"]]); flip[40] ^= 4
    proofs[t["flip"]] = bytes(flip)
    proofs[t["ident"]] = IDENT1
    proofs[t["undec"]] = b"\xff" * 64
    return t


@pytest.mark.parametrize("n", [1, 33, 70, 513])
def test_failed_proofs_make_bad_keys(eng, oracle, M, n):
    dst = M.DEFAULT_DST
    rnd = random.Random(310 + n)
    com = Committee(eng, n, 20 + n)
    proofs = proofs_of(eng, com, 20 + n)
    spoilt = tamper(com, proofs)
    pop = bits_of(eng.pop_verify_batch(com.pks, b"".join(proofs), n), n)
    failed = {i for i in range(n) if not pop[i]}
    assert set(spoilt.values()) <= failed
    if com.at:
        at = com.at
        assert {at["ident"], at["off"], at["undec"], at["nonsub"]} <= failed and not {at["p"], at["negp"], at["dup_a"], at["dup_b"]} & failed
        assert len(failed) == 8
    if n == 33:
        assert pop == bits_of(oracle.verify_batch(com.pks, list(com.keys), b"".join(proofs), M.POP_DST), n)
    rows, named = edge_rows(com, rnd)
    rows.append(set(range(n)) - failed - com.bad)                       # through the complement, the failed keys left unselected
    sel = [row_of(r, n) for r in rows]
    msgs = [b"checked %d/%d" % (n, g) for g in range(len(rows))]
    sigs = sign_rows(eng, com, rows, msgs, dst)
    msgs[named["tampered"]] += b"!"
    sigs[64 * named["ident_sig"]:64 * named["ident_sig"] + 64] = IDENT1
    sigs = bytes(sigs)
    # one small aggregation and one small merge: true signatures of keys with good and with spoilt proofs
    signers = [i for i in range(n) if com.sk[i]][:12]
    ag_msgs = [b"checked agg %d/%d" % (n, g) for g in range(3)]
    entries = []
    for g in range(3):
        ks_g = signers[g::3] if n > 1 else signers
        ss = eng.sign_batch(b"".join(b32(com.sk[i]) for i in ks_g), [ag_msgs[g]] * len(ks_g), dst)
        entries.append([(i, ss[64 * j:64 * j + 64]) for j, i in enumerate(ks_g)])
    clean = [i for i in signers if i not in failed]
    parts = [clean[0:3], [clean[3], min(set(signers) & failed)], clean[4:6]] if n > 1 else [signers]
    ps = sign_rows(eng, com, parts, [b"checked merge %d" % n] * len(parts), dst)
    contributions = [[(row_of(p, n), bytes(ps[64 * j:64 * j + 64])) for j, p in enumerate(parts)]]

    def calls(e, ks):
        return (ks.valid_bitmap(), e.keyset_sum_batch(ks, sel), e.keyset_fast_aggregate_verify_batch(ks, sel, msgs, sigs, dst),
                e.keyset_aggregate_checked_batch(ks, entries, ag_msgs, dst), e.keyset_merge_checked_batch(ks, contributions, [b"checked merge %d" % n], dst))

    plain = M.KeySet(eng, com.pks, n)
    stand_in = M.KeySet(eng, b"".join(UNDEC2 if i in failed else com.keys[i] for i in range(n)), n)
    checked = M.KeySet(eng, com.pks, n, proofs=b"".join(proofs))
    try:
        assert checked.checked() and not plain.checked() and checked.count() == n
        valid0 = bits_of(plain.valid_bitmap(), n)
        got, want = calls(eng, checked), calls(eng, stand_in)
    finally:
        plain.close(); stand_in.close(); checked.close()
    assert got[0] == synth.bitmap_of([valid0[i] and pop[i] for i in range(n)])
    assert got == want
    # what the comparison rests on: the spoilt keys do change results, and the complement leaves them out of the total
    out, status = got[1]
    assert list(status) == [0 if r & (failed | com.bad) else 1 for r in rows]
    fav = bits_of(got[2], len(rows))
    assert fav == [bool(r) and not r & failed and g not in (named["tampered"], named["ident_sig"]) and com.group_sk(r) == sum(com.sk[i] for i in r) % synth.R
                   for g, r in enumerate(rows)]
    last = rows[-1]
    if n > 1:
        assert 2 * len(last) > n and status[-1] == 1 and fav[-1] and sum(fav) >= 3
        assert out[-128:] == eng.aggregate_pks(com.gather(last), len(last))
    else:
        assert not last and out[-128:] == IDENT2 and not any(fav)
    ag_rows = got[3][1]
    rb = (n + 7) // 8
    for g, es in enumerate(entries):
        assert ag_rows[rb * g:rb * g + rb] == row_of([i for i, _ in es if i not in failed], n), g
    used = got[4][2][0]
    assert used == [not set(p) & failed for p in parts]


@pytest.mark.parametrize("n", [1, 70])
def test_proofs_that_all_hold_change_nothing(eng, M, n):
    dst = M.DEFAULT_DST
    rnd = random.Random(77)
    com = Committee(eng, n, 60 + n, special=False)
    proofs = eng.pop_prove_batch(b"".join(map(b32, com.sk)), n)
    rows, named = edge_rows(com, rnd)
    sel = [row_of(r, n) for r in rows]
    msgs = [b"all hold %d/%d" % (n, g) for g in range(len(rows))]
    sigs = bytes(sign_rows(eng, com, rows, msgs, dst))
    res = []
    for pf in (None, proofs):
        ks = M.KeySet(eng, com.pks, n, proofs=pf)
        try:
            res.append((ks.valid_bitmap(), eng.keyset_sum_batch(ks, sel), eng.keyset_fast_aggregate_verify_batch(ks, sel, msgs, sigs, dst)))
        finally:
            ks.close()
    assert res[0] == res[1] and res[0][0] == synth.bitmap_of([True] * n)
    assert bits_of(res[1][2], len(rows)) == [bool(r) for r in rows]


def test_argument_errors(eng, M):
    import ctypes
    import numpy as np
    lib, ctx = eng._lib, eng._ctx
    n = 3
    com = Committee(eng, n, 9, special=False)
    pks = np.frombuffer(com.pks, dtype=np.uint8)
    pf = np.frombuffer(eng.pop_prove_batch(b"".join(map(b32, com.sk)), n), dtype=np.uint8)
    u8 = ctypes.POINTER(ctypes.c_uint8)
    P = lambda a: a.ctypes.data_as(u8)
    tag = M.POP_DST

    def create(c=ctx, p=P(pks), q=P(pf), k=n, d=tag, dl=len(tag), out_h=True):
        h = ctypes.c_void_p(0x5a)
        return lib.blsbn254_keyset_create_checked(c, p, q, ctypes.c_size_t(k), d, ctypes.c_size_t(dl), ctypes.byref(h) if out_h else None), h

    for kw in ({"c": None}, {"p": None}, {"q": None}, {"k": 0}, {"k": 65537}, {"d": None}, {"out_h": False}):
        rc, h = create(**kw)
        assert rc == -1 and (not kw.get("out_h", True) or not h.value), kw
    rc, h = create()
    assert rc == 0 and lib.blsbn254_keyset_checked(h) == 1 and lib.blsbn254_keyset_checked(None) == 0
    bm = np.zeros(1, dtype=np.uint8)
    assert lib.blsbn254_keyset_valid(ctx, h, P(bm)) == 0 and bm[0] == 7
    lib.blsbn254_keyset_destroy(h)
    rc, h = create(d=b"another tag", dl=11)                             # every proof fails under another tag: not an error
    assert rc == 0 and lib.blsbn254_keyset_valid(ctx, h, P(bm)) == 0 and bm[0] == 0
    lib.blsbn254_keyset_destroy(h)
