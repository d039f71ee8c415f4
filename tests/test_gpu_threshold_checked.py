"""GPU tests (MI355X) of the checked threshold combine over ragged groups (blsbn254_threshold_combine_checked_batch): honest
groups against the oracle's signature under f(0), bad partials inside and outside the first t against the composition
verify_shares -> first t live shares -> combine, too few good partials, errors that cancel in the interpolation, bad groups that
stay local, launch boundaries, the argument errors, and call sequences on one context."""
import ctypes
import random

import numpy as np
import pytest

from tests import synth
from tests.gpu_support import eng, M
from tests.helpers import b32, bits_of, IDENT1, poly_eval
from tests.threshold_support import checked_flow, Deal, NEIGHBOUR_KEY, OTHER_MSG, pack

pytestmark = pytest.mark.gpu
R = synth.R
E_ARG = -1
ERR_SCALAR, ERR_G2, ST_SHORT = 1, 3, 5
SIZES_N = [1, 2, 5, 7, 64, 65, 3, 0]
SIZES_T = [1, 2, 3, 5, 33, 4, 5, 2]          # the last two groups are short by size
u8 = ctypes.POINTER(ctypes.c_uint8)
u64 = ctypes.POINTER(ctypes.c_uint64)


def composition(eng, deal):
    """what the parent offers: verify every share, take the first t live ones per group on the host, combine those"""
    commits, id_sets, sig_sets, msgs, dst = deal.args()
    bm, st = eng.threshold_verify_shares_batch(commits, id_sets, sig_sets, msgs, dst)
    assert st == bytes(deal.ng)
    ids_t, sigs_t, used = [], [], []
    for g in range(deal.ng):
        live = [i for i, b in enumerate(deal.group_bits(bm, g)) if b][:deal.ts[g]]
        enough = len(live) == deal.ts[g]
        used += [enough and i in live for i in range(deal.ns[g])]
        ids_t.append(b"".join(id_sets[g][32 * i:32 * i + 32] for i in live) if enough else b"")
        sigs_t.append(b"".join(sig_sets[g][64 * i:64 * i + 64] for i in live) if enough else b"")
    out, cst = eng.threshold_combine_batch(ids_t, sigs_t)
    assert cst == bytes(deal.ng)
    return bm, used, out


# ---------------------------------------------------------------- 1. all honest
@pytest.mark.parametrize("dst", [None, b"CHECKED-COMBINE-OTHER-DST"])
def test_all_honest(eng, oracle, M, dst):
    dst = M.DEFAULT_DST if dst is None else dst
    d = Deal(eng, SIZES_N, SIZES_T, 1, dst)
    s0 = eng.threshold_checked_stats()
    out, used, st = eng.threshold_combine_checked_batch(*d.args())
    s1 = eng.threshold_checked_stats()
    assert list(st) == [0] * 6 + [ST_SHORT] * 2
    for g in range(6):
        assert out[64 * g:64 * g + 64] == oracle.sign(d.coefs[g][0], d.msgs[g], dst), g
    assert out[64 * 6:] == IDENT1 * 2
    want_used = [g < 6 and i < d.ts[g] for g in range(8) for i in range(d.ns[g])]
    assert used == synth.bitmap_of(want_used)
    assert {k: s1[k] - s0[k] for k in s0} == {"optimistic_groups": 6, "fallback_groups": 0, "verified_shares": 0, "short_groups": 2}
    # offsets that do not start at 0: groups 2 .. 6 of the same arrays
    commits, id_sets, sig_sets, msgs, _ = d.args()
    ca = np.frombuffer(b"".join(commits), dtype=np.uint8); ia = np.frombuffer(b"".join(id_sets), dtype=np.uint8)
    sa = np.frombuffer(b"".join(sig_sets), dtype=np.uint8); ma = np.frombuffer(b"".join(msgs), dtype=np.uint8)
    da = np.frombuffer(dst, dtype=np.uint8)
    coff = np.cumsum([0] + SIZES_T).astype(np.uint64)[2:8]; goff = np.cumsum([0] + SIZES_N).astype(np.uint64)[2:8]
    moff = np.cumsum([0] + [len(m) for m in msgs]).astype(np.uint64)[2:8]
    n = int(goff[-1] - goff[0])
    o = np.full(64 * 5, 0x5a, dtype=np.uint8); ub = np.full((n + 7) // 8, 0x5a, dtype=np.uint8); s = np.full(5, 0x5a, dtype=np.uint8)
    rc = eng._lib.blsbn254_threshold_combine_checked_batch(eng._ctx, ca.ctypes.data_as(u8), coff.ctypes.data_as(u64), ia.ctypes.data_as(u8), sa.ctypes.data_as(u8),
                                                           goff.ctypes.data_as(u64), ma.ctypes.data_as(u8), moff.ctypes.data_as(u64), ctypes.c_size_t(5),
                                                           da.ctypes.data_as(u8), ctypes.c_size_t(len(dst)), o.ctypes.data_as(u8), ub.ctypes.data_as(u8),
                                                           s.ctypes.data_as(u8))
    assert rc == 0 and list(s) == [0] * 4 + [ST_SHORT]
    assert o.tobytes() == out[64 * 2:64 * 7]
    assert ub.tobytes() == synth.bitmap_of(want_used[int(goff[0]):int(goff[-1])])


# ---------------------------------------------------------------- 2. bad partials inside and outside the first t
def test_bad_partials_inside_and_outside_the_first_t(eng, oracle, M):
    dst = M.DEFAULT_DST
    ng = 30                                                          # groups 0 .. 24: position g % 5, kind g // 5; 25 .. 29 stay clean
    d = Deal(eng, [5] * ng, [3] * ng, 2, dst)
    for g in range(25):
        d.spoil(eng, g, g % 5, g // 5)
    bm, want_used, want_out = composition(eng, d)
    assert bits_of(bm, d.N) == [not (g < 25 and i == g % 5) for g in range(ng) for i in range(5)]
    s0 = eng.threshold_checked_stats()
    out, used, st = eng.threshold_combine_checked_batch(*d.args())
    s1 = eng.threshold_checked_stats()
    assert st == bytes(ng)
    assert used == synth.bitmap_of(want_used)
    assert out == want_out
    for g in range(ng):
        assert out[64 * g:64 * g + 64] == oracle.sign(d.coefs[g][0], d.msgs[g], dst), g
    # only a bad CANDIDATE among the first three candidates costs a fallback: kinds 0 and 1 at positions 0, 1, 2
    fallbacks = sum(1 for g in range(25) if g // 5 in (OTHER_MSG, NEIGHBOUR_KEY) and g % 5 < 3)
    assert fallbacks == 6
    assert s1["fallback_groups"] - s0["fallback_groups"] == fallbacks
    assert s1["verified_shares"] - s0["verified_shares"] == 5 * fallbacks
    assert s1["optimistic_groups"] - s0["optimistic_groups"] == ng - fallbacks and s1["short_groups"] == s0["short_groups"]


# ---------------------------------------------------------------- 3. too few good partials
def test_too_few_good_partials(eng, oracle, M):
    dst = M.DEFAULT_DST
    d = Deal(eng, [5] * 3, [3] * 3, 3, dst)
    for i in (0, 2, 4):
        d.spoil(eng, 1, i, OTHER_MSG)
    s0 = eng.threshold_checked_stats()
    out, used, st = eng.threshold_combine_checked_batch(*d.args())
    s1 = eng.threshold_checked_stats()
    assert list(st) == [0, ST_SHORT, 0]
    assert out[64:128] == IDENT1
    assert used == synth.bitmap_of([True] * 3 + [False] * 2 + [False] * 5 + [True] * 3 + [False] * 2)
    for g in (0, 2):
        assert out[64 * g:64 * g + 64] == oracle.sign(d.coefs[g][0], d.msgs[g], dst), g
    assert {k: s1[k] - s0[k] for k in s0} == {"optimistic_groups": 2, "fallback_groups": 1, "verified_shares": 5, "short_groups": 1}


# ---------------------------------------------------------------- 4. cancelling errors
def test_cancelling_errors(eng, oracle, M):
    dst = M.DEFAULT_DST
    d = Deal(eng, [4, 4], [3, 3], 4, dst, small_ids=True)
    lam, lst = eng.lagrange_at_zero_batch([b32(1) + b32(2) + b32(3)])
    assert lst == bytes(1)
    l0, l1 = int.from_bytes(lam[:32], "big"), int.from_bytes(lam[32:64], "big")
    a = random.Random(44).randrange(1, R)
    b = (-l0 * a) * pow(l1, -1, R) % R
    assert (l0 * a + l1 * b) % R == 0 and b != 0
    P = oracle.g1_generator()
    deltas = eng.g1_mul_batch(P * 2, b32(a) + b32(b), 2)
    for i in (0, 1):                                                 # group 0: partials 0 and 1 shifted by [a] P and [b] P
        d.sigs[64 * i:64 * i + 64] = oracle.g1_add(bytes(d.sigs[64 * i:64 * i + 64]), deltas[64 * i:64 * i + 64])
    s0 = eng.threshold_checked_stats()
    out, used, st = eng.threshold_combine_checked_batch(*d.args())
    s1 = eng.threshold_checked_stats()
    assert st == bytes(2)
    for g in (0, 1):
        assert out[64 * g:64 * g + 64] == oracle.sign(d.coefs[g][0], d.msgs[g], dst), g
    assert used == synth.bitmap_of([True, True, True, False] * 2)
    assert s1["fallback_groups"] == s0["fallback_groups"] and s1["verified_shares"] == s0["verified_shares"]
    bm, vst = eng.threshold_verify_shares_batch(*d.args())
    assert vst == bytes(2) and bm == synth.bitmap_of([False, False, True, True] + [True] * 4)


# ---------------------------------------------------------------- 5. bad groups stay local
def test_bad_groups_stay_local(eng, M):
    dst = M.DEFAULT_DST
    d = Deal(eng, [5] * 8, [3] * 8, 5, dst, small_ids=True)
    rnd = random.Random(55)
    d.ids = [rnd.sample(range(1, 1000), 5) for _ in range(8)]
    d.shares = [poly_eval(d.coefs[g], x) for g in range(8) for x in d.ids[g]]
    d.sigs = bytearray(d.sign(eng, d.shares, [d.msgs[g] for g in range(8) for _ in range(5)]))
    good = [4, 6, 7]
    alone = eng.threshold_combine_checked_batch(*d.args(good))
    assert alone[2] == bytes(3) and alone[1] == synth.bitmap_of([True, True, True, False, False] * 3)
    d.commits[0] = d.commits[0][:256] + synth.NON_SUBGROUP_PK        # outside the subgroup
    d.ids[1][1] = 0                                                  # id == 0
    d.ids[2][0] = R                                                  # id == r
    d.ids[3][4] = d.ids[3][0]                                        # repeated, beyond the first t
    d.ids[5][4] = R; d.commits[5] = b"\xff" * 128 + d.commits[5][128:]   # both: the scalar error wins
    want = {0: ERR_G2, 1: ERR_SCALAR, 2: ERR_SCALAR, 3: ERR_SCALAR, 5: ERR_SCALAR}
    out, used, st = eng.threshold_combine_checked_batch(*d.args())
    assert list(st) == [want.get(g, 0) for g in range(8)]
    for g in want:
        assert out[64 * g:64 * g + 64] == IDENT1 and d.group_bits(used, g) == [False] * 5, g
    for k, g in enumerate(good):
        assert out[64 * g:64 * g + 64] == alone[0][64 * k:64 * k + 64], g
        assert d.group_bits(used, g) == [True, True, True, False, False], g


def test_several_launches(eng, M, monkeypatch):
    dst = M.DEFAULT_DST
    ng = 1 << 10
    d = checked_flow(eng, ng, 16, 6, dst)
    s0 = eng.threshold_checked_stats()
    got = eng.threshold_combine_checked_batch(*d.args())
    s1 = eng.threshold_checked_stats()
    assert got[2] == bytes(ng) and s1["fallback_groups"] - s0["fallback_groups"] == ng // 16
    c0 = b"".join(c[:128] for c in d.commits)
    assert eng.verify_batch(c0, d.msgs, got[0], dst) == synth.bitmap_of([True] * ng)
    bad = {5 * g + (g // 16) % 3 for g in range(0, ng, 16)}
    want_used = []
    for g in range(ng):
        live = [i for i in range(5) if 5 * g + i not in bad][:3]
        want_used += [i in live for i in range(5)]
    assert got[1] == synth.bitmap_of(want_used)
    with monkeypatch.context() as mp:                                # more than one launch chunk, none ending on a group boundary
        mp.setenv("BLSBN254_CHUNK_LANES", "4104")
        e2 = M.Engine(0)
        try:
            assert e2.threshold_combine_checked_batch(*d.args()) == got
        finally:
            e2.close()


# ---------------------------------------------------------------- 7. argument errors
def test_argument_errors(eng, M):
    lib, ctx = eng._lib, eng._ctx
    d = Deal(eng, [2, 2], [2, 2], 7, b"TEST", small_ids=True)
    commits = np.frombuffer(b"".join(d.commits), dtype=np.uint8)
    big = 4099
    ids = np.zeros(32 * big, dtype=np.uint8); ids[:32 * 4] = np.frombuffer(b"".join(pack(d.ids)), dtype=np.uint8)
    sigs = np.zeros(64 * big, dtype=np.uint8); sigs[:64 * 4] = np.frombuffer(bytes(d.sigs), dtype=np.uint8)
    msgs = np.frombuffer(b"".join(d.msgs), dtype=np.uint8)
    ml = len(d.msgs[0])
    out = np.zeros(64 * 2, dtype=np.uint8); used = np.zeros((big + 7) // 8, dtype=np.uint8); st = np.zeros(2, dtype=np.uint8)
    P = lambda a: a.ctypes.data_as(u8)
    keep = []

    def off(o):
        if o is None:
            return None
        a = np.ascontiguousarray(np.asarray(o, dtype=np.uint64)); keep.append(a)
        return a.ctypes.data_as(u64)

    def cc(coff=(0, 2, 4), goff=(0, 2, 4), n=2, c=ctx, a=P(commits), i=P(ids), s=P(sigs), m=P(msgs), moff=(0, ml, 2 * ml), dst=b"TEST", dl=4, o=P(out), u=P(used),
           t=P(st)):
        return lib.blsbn254_threshold_combine_checked_batch(c, a, off(coff), i, s, off(goff), m, off(moff), ctypes.c_size_t(n), dst, ctypes.c_size_t(dl), o, u, t)

    assert cc() == 0 and st.tobytes() == bytes(2) and used[0] == 0x0f
    assert eng.verify_batch(d.commits[0][:128] + d.commits[1][:128], d.msgs, out.tobytes(), b"TEST") == b"\x03"
    assert cc(coff=(0, 3, 1)) == E_ARG and cc(goff=(0, 3, 1)) == E_ARG and cc(moff=(0, 3, 1)) == E_ARG     # decreasing offsets
    assert cc(goff=(0, 1, (1 << 23) + 1)) == E_ARG and cc(coff=(0, 1, (1 << 23) + 1)) == E_ARG
    for name in ("c", "a", "i", "s", "m", "dst", "o", "u", "t", "coff", "goff", "moff"):
        assert cc(**{name: None}) == E_ARG, name
    assert cc(goff=(0, 2, 4099)) == E_ARG and b"group" in lib.blsbn254_last_error(ctx)                  # a group of 4097 shares
    assert cc(goff=(0, 4096, 4098)) == 0                                                                # 4096 are served
    assert cc(n=0) == 0 and cc(coff=None, goff=None, moff=None, n=0, a=None, i=None, s=None, m=None, o=None, u=None, t=None) == 0
    assert cc(m=None, moff=(0, 0, 0)) == 0 and cc(dst=None, dl=0) == 0
    out[:] = 0x5a; st[:] = 0x5a
    assert cc(goff=(0, 0, 0), i=None, s=None, u=None) == 0                                              # no shares at all
    assert list(st) == [ST_SHORT] * 2 and out.tobytes() == IDENT1 * 2
    assert cc(coff=(0, 0, 0), a=None) == 0 and list(st) == [ST_SHORT] * 2                               # no thresholds at all
    assert lib.blsbn254_threshold_checked_stats(ctx, None) == E_ARG and lib.blsbn254_threshold_checked_stats(None, (ctypes.c_uint64 * 4)()) == E_ARG
    assert lib.blsbn254_strerror(ST_SHORT) not in (lib.blsbn254_strerror(99), lib.blsbn254_strerror(4)) and M.ST_SHORT == ST_SHORT
    assert eng.threshold_combine_checked_batch([], [], [], [], b"TEST") == (b"", b"", b"")
    with pytest.raises(ValueError):
        eng.threshold_combine_checked_batch([bytes(128)], [bytes(32)], [bytes(128)], [b""], b"TEST")
    with pytest.raises(ValueError):
        eng.threshold_combine_checked_batch([bytes(128)], [bytes(32)], [bytes(64)], [], b"TEST")


# ---------------------------------------------------------------- 8. call sequences on one context
def test_call_sequences_on_one_context(M, eng, oracle):
    dst, dst2 = M.DEFAULT_DST, b"CHECKED-COMBINE-SECOND-DST"
    vb = synth.make_batch_gpu(eng, oracle, 600, dst, pool=40, invalid_every=7, spot=4)          # repeated keys: the prepared path
    d1, d2 = checked_flow(eng, 96, 8, 8, dst), checked_flow(eng, 40, 4, 9, dst2)
    a1, a2 = d1.args(), d2.args()
    ids3 = [b32(1) + b32(3) + b32(5)] * 96
    sigs3 = [s[:64] + s[128:192] + s[256:320] for s in a1[2]]
    steps = [
        lambda e: e.threshold_combine_checked_batch(*a1),
        lambda e: e.verify_batch(vb[0], vb[1], vb[2], dst),
        lambda e: e.threshold_combine_checked_batch(*a2),
        lambda e: e.threshold_combine_batch(ids3, sigs3),
        lambda e: e.g2_poly_eval_batch(a1[0], a1[1]),
        lambda e: e.threshold_combine_checked_batch(*a1),
        lambda e: e.verify_batch(vb[0], vb[1], vb[2], dst),
    ]
    fresh = []
    for f in steps:
        e = M.Engine(0)
        try:
            fresh.append(f(e))
        finally:
            e.close()
    assert fresh[0][2] == bytes(96) and fresh[2][2] == bytes(40) and fresh[1] == synth.bitmap_of(vb[3])
    assert eng.verify_batch(b"".join(c[:128] for c in a2[0]), a2[3], fresh[2][0], dst2) == synth.bitmap_of([True] * 40)
    e = M.Engine(0)
    try:
        got = [f(e) for f in steps]
        assert e.threshold_checked_stats()["fallback_groups"] == 12 + 10 + 12
    finally:
        e.close()
    for k, (a, b) in enumerate(zip(got, fresh)):
        assert a == b, "step %d differs from the same call on a context of its own" % k
