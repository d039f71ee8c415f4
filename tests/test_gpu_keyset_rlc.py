"""GPU tests (MI355X) of the key-set FastAggregateVerify by random linear combination per message
(blsbn254_keyset_fast_aggregate_verify_batch_rlc, its committee form, blsbn254_set_keyset_rlc_group, blsbn254_keyset_rlc_stats).
Expected bits always come from the EXACT call on the same arguments, and where a closed form exists (a signature made with the sum
of the selected secret keys verifies; a tampered one does not) from that too -- never from the call under test.  Every case runs
under three fixed seeds and under seed = None."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

import blsbn254_loader
from tests import synth
from tests.gpu_support import eng, M
from tests.helpers import b32, bits_of, IDENT1, row_of
from tests.keyset_support import Committee, rlc_model_plan, sign_rows

pytestmark = pytest.mark.gpu
E_ARG = -1
_M = blsbn254_loader.load()
_M.Engine.keyset_fast_aggregate_verify_batch_rlc, _M.Engine.keyset_rlc_stats         # the feature is there, or this module does not import
DST = _M.DEFAULT_DST
SEEDS = [b"\x01" * 32, bytes(range(32)), hashlib.sha256(b"key-set rlc").digest(), None]
N = 70


@pytest.fixture(scope="module")
def reg(eng):
    return Committee(eng, N, 71)


@pytest.fixture(scope="module")
def ks(eng, M, reg):
    k = M.KeySet(eng, reg.pks, N)
    yield k
    k.close()


@pytest.fixture(scope="module")
def one_class(eng, reg):
    """129 groups of good keys that sign ONE message: (sets, rows, message, signatures); every prefix is a case of its own"""
    rnd = random.Random(129)
    good = [i for i in range(N) if i not in reg.unsignable]
    sets = [{i for i in good if rnd.random() < (0.3, 0.7)[g & 1]} | {good[g % len(good)]} for g in range(129)]
    msg = b"one message for the whole slot"
    sigs = bytes(sign_rows(eng, reg, sets, [msg] * 129, DST))
    return sets, [row_of(s, N) for s in sets], msg, sigs


def delta(eng, f):
    s0 = eng.keyset_rlc_stats()
    out = f()
    s1 = eng.keyset_rlc_stats()
    return out, {k: s1[k] - s0[k] for k in s1}


def neg_g1(p):
    return p[:32] + b32(synth.P - int.from_bytes(p[32:], "big"))


def chunk_model(msgs, C):
    """(chunks worth checking when every group is eligible, groups in them, groups alone in their chunk)"""
    _, chunks, rep = rlc_model_plan(msgs, C)
    multi = [l for _, l, _ in chunks if l >= 2]
    return len(multi), sum(multi), sum(1 for _, l, _ in chunks if l == 1), len(rep)


@pytest.mark.parametrize("C", [64, 2])
def test_all_valid(eng, ks, one_class, C):
    sets, rows, msg, sigs = one_class
    eng.set_keyset_rlc_group(0 if C == 64 else C)
    try:
        for size in (1, 2, 63, 64, 65, 129):
            msgs = [msg] * size
            want = eng.keyset_fast_aggregate_verify_batch(ks, rows[:size], msgs, sigs[:64 * size], DST)
            assert want == synth.bitmap_of([True] * size)               # closed form: signed with the sum of the selected secret keys
            n_chunks, in_chunks, alone, n_cls = chunk_model(msgs, C)
            assert n_cls == 1 and alone == (size % C == 1) and in_chunks + alone == size
            for seed in SEEDS:
                got, d = delta(eng, lambda: eng.keyset_fast_aggregate_verify_batch_rlc(ks, rows[:size], msgs, sigs[:64 * size], DST, seed))
                assert got == want, (size, seed)
                assert d == {"decided_groups": in_chunks, "chunks": n_chunks, "failed_chunk_groups": 0, "direct_groups": alone, "classes": 1, "calls": 1}, (size, d)
    finally:
        eng.set_keyset_rlc_group(0)


def test_one_wrong_signature(eng, ks, reg, one_class):
    sets, rows, msg, sigs = one_class
    bad = 70                                                            # in the second chunk of 64
    other = bytes(sign_rows(eng, reg, [sets[bad]], [b"another message"], DST))
    sigs = sigs[:64 * bad] + other + sigs[64 * bad + 64:]
    msgs = [msg] * 129
    want = eng.keyset_fast_aggregate_verify_batch(ks, rows, msgs, sigs, DST)
    assert want == synth.bitmap_of([g != bad for g in range(129)])
    for seed in SEEDS:
        got, d = delta(eng, lambda: eng.keyset_fast_aggregate_verify_batch_rlc(ks, rows, msgs, sigs, DST, seed))
        assert got == want
        assert d == {"decided_groups": 64, "chunks": 2, "failed_chunk_groups": 64, "direct_groups": 1, "classes": 1, "calls": 1}


def test_cancelling_errors(eng, ks, reg, one_class):
    """Two groups of ONE chunk carry sig_a + D and sig_b - D: the plain sum of the chunk's signatures is unchanged, so a
    combination WITHOUT weights (every r_g = 1) would pass the chunk and set both bits.  The exact call clears both, and so must
    this call under every seed: THIS is the test that shows the weights are applied."""
    sets, rows, msg, sigs = one_class
    a, b = 3, 40
    D = bytes(sign_rows(eng, reg, [{0}], [b"the error term"], DST))
    sa = eng.aggregate_sigs(sigs[64 * a:64 * a + 64] + D, 2)
    sb = eng.aggregate_sigs(sigs[64 * b:64 * b + 64] + neg_g1(D), 2)
    bad = bytearray(sigs[:64 * 64])
    bad[64 * a:64 * a + 64] = sa; bad[64 * b:64 * b + 64] = sb
    bad = bytes(bad)
    assert eng.aggregate_sigs(bad, 64) == eng.aggregate_sigs(sigs[:64 * 64], 64)      # the errors cancel in the unweighted sum
    msgs = [msg] * 64
    want = eng.keyset_fast_aggregate_verify_batch(ks, rows[:64], msgs, bad, DST)
    assert want == synth.bitmap_of([g not in (a, b) for g in range(64)])
    for seed in SEEDS:
        got, d = delta(eng, lambda: eng.keyset_fast_aggregate_verify_batch_rlc(ks, rows[:64], msgs, bad, DST, seed))
        assert got == want, seed
        assert d["chunks"] == 1 and d["failed_chunk_groups"] == 64 and d["decided_groups"] == 0


def test_several_classes(eng, ks, reg):
    """classes interleaved in the caller's order, one of a single group, two that differ in the last message byte only"""
    rnd = random.Random(4)
    good = [i for i in range(N) if i not in reg.unsignable]
    msgs = [b"class A"] * 30 + [b"class B"] * 5 + [b"single"] + [b"slot 7a"] * 4 + [b"slot 7b"] * 3
    rnd.shuffle(msgs)
    G = len(msgs)
    sets = [set(rnd.sample(good, rnd.randrange(1, 40))) for _ in range(G)]
    sigs = bytearray(sign_rows(eng, reg, sets, msgs, DST))
    wrong = [g for g in range(G) if msgs[g] == b"class B"][2]
    sigs[64 * wrong:64 * wrong + 64] = sign_rows(eng, reg, [sets[wrong]], [b"class b"], DST)
    swapped = [g for g in range(G) if msgs[g] == b"slot 7a"][0]         # signed for the neighbouring class
    sigs[64 * swapped:64 * swapped + 64] = sign_rows(eng, reg, [sets[swapped]], [b"slot 7b"], DST)
    sigs = bytes(sigs)
    rows = [row_of(s, N) for s in sets]
    want = eng.keyset_fast_aggregate_verify_batch(ks, rows, msgs, sigs, DST)
    assert want == synth.bitmap_of([g not in (wrong, swapped) for g in range(G)])
    assert sum(1 for x, y in zip(msgs, msgs[1:]) if x != y) > 10
    for seed in SEEDS:
        got, d = delta(eng, lambda: eng.keyset_fast_aggregate_verify_batch_rlc(ks, rows, msgs, sigs, DST, seed))
        assert got == want
        assert d == {"decided_groups": 30 + 3, "chunks": 4, "failed_chunk_groups": 5 + 4, "direct_groups": 1, "classes": 5, "calls": 1}


def test_every_ineligible_kind_beside_valid_groups(eng, ks, reg):
    at = reg.at
    rnd = random.Random(6)
    good = [i for i in range(N) if i not in reg.unsignable and i not in (at["p"], at["negp"], at["ident"])]
    valid_sets = [set(rnd.sample(good, rnd.randrange(1, 30))) for _ in range(10)]
    sets = list(valid_sets)
    kinds = {}
    for name, s in (("empty", set()), ("bad", {0, at["off"]}), ("undec", {at["undec"], 2}), ("nonsub", {0, at["nonsub"]}), ("p_negp", {at["p"], at["negp"]}),
                    ("p_negp_third", {at["p"], at["negp"], 11}), ("with_ident_key", {0, 2, at["ident"]}), ("ident_sig", set(good[:9])), ("undec_sig", set(good[3:9])),
                    ("off_curve_sig", set(good[5:20]))):
        kinds[name] = len(sets); sets.append(s)
    order = list(range(len(sets)))
    rnd.shuffle(order)
    sets = [sets[i] for i in order]
    where = {name: order.index(i) for name, i in kinds.items()}
    G = len(sets)
    msgs = [b"the one message"] * G
    sigs = bytearray(sign_rows(eng, reg, sets, msgs, DST))
    g = where["ident_sig"]; sigs[64 * g:64 * g + 64] = IDENT1
    g = where["undec_sig"]; sigs[64 * g:64 * g + 32] = b"\xff" * 32
    g = where["off_curve_sig"]; sigs[64 * g + 63] ^= 1
    sigs = bytes(sigs)
    rows = [row_of(s, N) for s in sets]
    want = eng.keyset_fast_aggregate_verify_batch(ks, rows, msgs, sigs, DST)
    cleared = {where[k] for k in ("empty", "bad", "undec", "nonsub", "p_negp", "ident_sig", "undec_sig", "off_curve_sig")}
    assert want == synth.bitmap_of([g not in cleared for g in range(G)])            # closed form
    for seed in SEEDS:
        got, d = delta(eng, lambda: eng.keyset_fast_aggregate_verify_batch_rlc(ks, rows, msgs, sigs, DST, seed))
        assert got == want
        # the ten valid groups and the two eligible edge rows pass by combination; the eight others take the exact path directly
        assert d == {"decided_groups": 12, "chunks": 1, "failed_chunk_groups": 0, "direct_groups": 8, "classes": 1, "calls": 1}


def test_a_chunk_with_one_eligible_member(eng, ks, one_class):
    """what can be constructed deterministically of a chunk that is not checked: one eligible member (state 0).  A weighted sum
    that is the identity (state 2) is covered by the lane function in tests/test_keyset_rlc_host.py."""
    sets, rows, msg, sigs = one_class
    s2 = sigs[:64] + IDENT1
    want = eng.keyset_fast_aggregate_verify_batch(ks, rows[:2], [msg] * 2, s2, DST)
    assert want == b"\x01"
    for seed in SEEDS:
        got, d = delta(eng, lambda: eng.keyset_fast_aggregate_verify_batch_rlc(ks, rows[:2], [msg] * 2, s2, DST, seed))
        assert got == want
        assert d == {"decided_groups": 0, "chunks": 0, "failed_chunk_groups": 0, "direct_groups": 2, "classes": 1, "calls": 1}


def test_committee_form(eng, M, reg):
    at = reg.at
    rnd = random.Random(8)
    coms = [[20], list(range(10, 41)), list(range(24, 56)), list(range(69, 36, -1)), list(range(0, 65)), [0, at["nonsub"], 33]]
    assert [len(c) for c in coms] == [1, 31, 32, 33, 65, 3] and at["undec"] in coms[3] and at["off"] in coms[4]
    groups = []                                                         # (committee, member positions)
    for c, mem in enumerate(coms):
        clean = [j for j, i in enumerate(mem) if i not in reg.unsignable]
        for _ in range(6):
            groups.append((c, set(rnd.sample(clean, rnd.randrange(1, len(clean) + 1)))))
        groups.append((c, set(clean)))                                  # more than half: through the complement
    groups.append((5, {0, 1}))                                          # selects the key outside the r-torsion: not eligible
    groups.append((5, {1}))
    groups.append((4, {at["off"], 0}))                                  # selects a bad key
    groups.append((3, {coms[3].index(at["undec"]), 0}))
    groups.append((1, set()))
    rnd.shuffle(groups)
    G = len(groups)
    com = [c for c, _ in groups]
    rows = [row_of(r, len(coms[c])) for c, r in groups]
    sets = [{coms[c][j] for j in r} for c, r in groups]
    msgs = [(b"slot 11", b"slot 12")[g % 3 == 0] for g in range(G)]     # groups of several committees share one message
    sigs = bytearray(sign_rows(eng, reg, sets, msgs, DST))
    tampered = next(g for g in range(G) if sets[g] and not (sets[g] & reg.unsignable) and msgs[g] == b"slot 11")
    sigs[64 * tampered:64 * tampered + 64] = sign_rows(eng, reg, [sets[tampered]], [b"slot 12"], DST)
    sigs = bytes(sigs)
    k = M.KeySet(eng, reg.pks, N)
    try:
        k.set_committees(coms)
        want = eng.keyset_committee_fast_aggregate_verify_batch(k, com, rows, msgs, sigs, DST)
        expect = [bool(sets[g] - {at["ident"]}) and not (sets[g] & reg.unsignable) and g != tampered and sets[g] != {at["p"], at["negp"]} for g in range(G)]
        assert want == synth.bitmap_of(expect) and sum(expect) > 30 and G - sum(expect) >= 6
        c0, f0 = eng.keyset_committee_stats(), eng.keyset_stats()
        for seed in SEEDS:
            got, d = delta(eng, lambda: eng.keyset_committee_fast_aggregate_verify_batch_rlc(k, com, rows, msgs, sigs, DST, seed))
            assert got == want
            assert d["classes"] == 2 and d["chunks"] == 2 and d["calls"] == 1 and d["decided_groups"] + d["failed_chunk_groups"] + d["direct_groups"] == G
            assert d["decided_groups"] == sum(1 for g in range(G) if expect[g] and msgs[g] == b"slot 12")     # the chunk of "slot 11" fails
        c1 = eng.keyset_committee_stats()
        assert c1["groups"] - c0["groups"] == len(SEEDS) * G and eng.keyset_stats() == f0      # the sums are counted as the exact call counts them
    finally:
        k.close()


def test_call_sequences_on_one_context(M, eng, oracle, reg, one_class):
    """the RLC call between an exact key-set call, a verify_batch with another tag and a second RLC call with another C: each
    result equals the same call on a fresh context"""
    sets, rows, msg, sigs = one_class
    msgs = [msg if g % 4 else b"the other message" for g in range(129)]
    sg = bytearray(sign_rows(eng, reg, sets, msgs, DST))
    sg[64 * 9 + 63] ^= 1; sg[64 * 77:64 * 77 + 64] = sg[64 * 78:64 * 78 + 64]
    sg = bytes(sg)
    dst2 = DST[:-1] + bytes([DST[-1] ^ 1])
    vb = synth.make_batch_gpu(eng, oracle, 300, dst2, pool=20, invalid_every=7, spot=2)
    seed = SEEDS[1]

    def exact(e, k):
        return e.keyset_fast_aggregate_verify_batch(k, rows, msgs, sg, DST)

    def rlc(e, k):
        e.set_keyset_rlc_group(0)
        return e.keyset_fast_aggregate_verify_batch_rlc(k, rows, msgs, sg, DST, seed), e.keyset_rlc_stats()["chunks"]

    def rlc2(e, k):
        e.set_keyset_rlc_group(2)
        return e.keyset_fast_aggregate_verify_batch_rlc(k, rows, msgs, sg, DST, seed), e.keyset_rlc_stats()["chunks"]

    def verify(e, k):
        return e.verify_batch(vb[0], vb[1], vb[2], dst2)

    def run(seq):
        e = M.Engine(0)
        try:
            k = M.KeySet(e, reg.pks, N)
            out, chunks = [], 0
            for f in seq:
                r = f(e, k)
                if f in (rlc, rlc2):                                    # the counter is cumulative: compare what this call added
                    r, chunks = (r[0], r[1] - chunks), r[1]
                out.append(r)
            k.close()
            return out
        finally:
            e.close()

    alone = {f: run([f])[0] for f in (exact, rlc, rlc2, verify)}
    assert alone[rlc][0] == alone[exact] == alone[rlc2][0] and alone[verify] == synth.bitmap_of(vb[3])
    # C = 64: 33 + 96 groups in 1 + 2 chunks; C = 2: 16 + 48 pairs, and the pair of group 9 (an off-curve signature) has one eligible member
    assert alone[rlc][1] == 3 and alone[rlc2][1] == 63 and not bits_of(alone[exact], 129)[9] and not bits_of(alone[exact], 129)[77]
    seq = [exact, rlc, verify, rlc2, rlc, exact, rlc2]
    assert run(seq) == [alone[f] for f in seq]


def test_argument_errors(eng, M, reg):
    lib, ctx = eng._lib, eng._ctx
    u8, u32, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    n = 13                                                              # rows of 2 bytes, 3 padding bits
    com = Committee(eng, n, 72)
    sets = [{0, 1, 12}, set(range(n)), {5}]
    msgs = [b"a", b"a", b"def"]
    sigs = bytes(sign_rows(eng, com, sets, msgs, b"TEST"))
    sel = np.frombuffer(b"".join(row_of(r, n) for r in sets), dtype=np.uint8).copy()
    data = np.frombuffer(b"".join(msgs), dtype=np.uint8)
    off = np.array([0, 1, 2, 5], dtype=np.uint64)
    sg = np.frombuffer(sigs, dtype=np.uint8)
    bm = np.zeros(1, dtype=np.uint8)
    seed = np.frombuffer(SEEDS[0], dtype=np.uint8)
    P = lambda a: a.ctypes.data_as(u8)
    ks = M.KeySet(eng, com.pks, n)
    h = ks._h

    def fav(c=ctx, k=h, s=P(sel), m=P(data), of=off.ctypes.data_as(u64), sig=P(sg), g=3, d=b"TEST", dl=4, sd=P(seed), b=P(bm)):
        return lib.blsbn254_keyset_fast_aggregate_verify_batch_rlc(c, k, s, m, of, sig, ctypes.c_size_t(g), d, ctypes.c_size_t(dl), sd, b)

    cm = np.array([0, 1, 0], dtype=np.uint32)
    csel = np.frombuffer(row_of([0, 12], 13) + row_of([15], 16) + row_of(range(13), 13), dtype=np.uint8).copy()
    so = np.array([0, 2, 4, 6], dtype=np.uint64)

    def cfav(c=ctx, k=h, cc=cm, s=csel, o=so, g=3):
        return lib.blsbn254_keyset_committee_fast_aggregate_verify_batch_rlc(c, k, cc.ctypes.data_as(u32), P(s), o.ctypes.data_as(u64), P(data), off.ctypes.data_as(u64),
                                                                             P(sg), ctypes.c_size_t(g), b"TEST", ctypes.c_size_t(4), P(seed), P(bm))

    try:
        assert fav() == 0 and bm[0] == 7 and fav(sd=None) == 0 and bm[0] == 7
        served = eng.keyset_rlc_stats()
        eng.profile_enable(True); eng.profile_reset()
        for name in ("c", "k", "s", "of", "sig", "d", "b"):             # those of the exact call
            assert fav(**{name: None}) == E_ARG, name
        assert fav(g=0) == 0 and fav(g=0, s=None, sig=None, b=None) == 0
        assert fav(m=None) == E_ARG                                     # messages of non-zero length and no bytes
        down = np.array([0, 2, 1, 5], dtype=np.uint64)
        assert fav(of=down.ctypes.data_as(u64)) == E_ARG
        e2 = M.Engine(0)                                                # a key set that belongs to another context
        try:
            assert fav(c=e2._ctx) == E_ARG
        finally:
            e2.close()
        for g, bit in ((0, 5), (2, 7)):                                 # a padding bit in a row's last byte
            sel[2 * g + 1] ^= 1 << bit
            assert fav() == E_ARG and b"row %d" % g in lib.blsbn254_last_error(ctx)
            sel[2 * g + 1] ^= 1 << bit
        assert cfav() == E_ARG and b"no committees" in lib.blsbn254_last_error(ctx)
        for group in (1, 4097, 1 << 20):
            assert lib.blsbn254_set_keyset_rlc_group(ctx, ctypes.c_size_t(group)) == E_ARG
            with pytest.raises(M.Bn254Error):
                eng.set_keyset_rlc_group(group)
        assert lib.blsbn254_set_keyset_rlc_group(None, ctypes.c_size_t(2)) == E_ARG
        assert lib.blsbn254_keyset_rlc_stats(ctx, None) == E_ARG and lib.blsbn254_keyset_rlc_stats(None, (ctypes.c_uint64 * 6)()) == E_ARG
        launched = eng.profile_read()
        eng.profile_enable(False); eng.profile_reset()
        assert launched == {} and eng.keyset_rlc_stats() == served       # the refused calls launched nothing
        for group in (2, 4096, 0):
            eng.set_keyset_rlc_group(group)
            bm[:] = 0
            assert fav() == 0 and bm[0] == 7
        ks.set_committees([list(range(13))])
        assert cfav(cc=np.array([0, 1, 0], dtype=np.uint32)) == E_ARG and b"group 1" in lib.blsbn254_last_error(ctx)      # com[g] = n_com
        assert cfav(cc=np.array([0, 0, 0], dtype=np.uint32), o=np.array([0, 2, 3, 5], dtype=np.uint64)) == E_ARG and b"group 1" in lib.blsbn254_last_error(ctx)
        assert cfav(g=0) == 0
        with pytest.raises(ValueError):
            eng.keyset_fast_aggregate_verify_batch_rlc(ks, [bytes(2)], [], b"", b"TEST")
        with pytest.raises(ValueError):
            eng.keyset_fast_aggregate_verify_batch_rlc(ks, [bytes(2)], [b"m"], bytes(64), b"TEST", seed=b"short")
        assert eng.keyset_fast_aggregate_verify_batch_rlc(ks, [], [], b"", b"TEST") == b""
    finally:
        eng.set_keyset_rlc_group(0)
        ks.close()
