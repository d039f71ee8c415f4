"""GPU tests (MI355X) of the check of dealt key shares against Feldman commitments over ragged groups
(blsbn254_threshold_verify_key_shares_batch): against a Python Horner and against the composition it replaces
(sk_to_pk_batch of the shares == g2_poly_eval_batch, byte for byte), wrong shares of every kind that clear their own bit only,
the zero share and the empty polynomial, bad groups that stay local, launches that end inside groups, the life of the generator
table on a context, and the argument errors."""
import ctypes
import random

import numpy as np
import pytest

from tests import synth
from tests.gpu_support import eng, M  # noqa: F401 (fixtures)
from tests.helpers import b32, bits_of, poly_eval

pytestmark = pytest.mark.gpu
R = synth.R
E_ARG = -1
ERR_SCALAR, ERR_G2 = 1, 3
SIZES_N = [1, 2, 0, 7, 63, 64, 65, 257]
SIZES_T = [1, 2, 3, 8, 33, 0, 5, 4]
u8 = ctypes.POINTER(ctypes.c_uint8)
u64 = ctypes.POINTER(ctypes.c_uint64)


def pack(sets):
    return [b"".join(map(b32, s)) for s in sets]


def commitments(eng, coef_sets):
    flat = [c for s in coef_sets for c in s]
    pks = eng.sk_to_pk_batch(b"".join(map(b32, flat)), len(flat)) if flat else b""
    out, pos = [], 0
    for s in coef_sets:
        out.append(pks[128 * pos:128 * (pos + len(s))])
        pos += len(s)
    return out


def composition(eng, commits, id_sets, share_sets):
    """the parent's way to the same bits: [share] G2gen by sk_to_pk_batch, the key shares by g2_poly_eval_batch, a byte compare"""
    flat = b"".join(share_sets)
    n = len(flat) // 32
    lhs = eng.sk_to_pk_batch(flat, n)
    rhs, st = eng.g2_poly_eval_batch(commits, id_sets)
    return [lhs[128 * i:128 * i + 128] == rhs[128 * i:128 * i + 128] for i in range(n)], st


def small_groups(eng, n_groups, seed, n=7, t=5):
    """n_groups x (ids 1 .. n, t coefficients): coefficients, packed ids, commitments, the honest shares as integers"""
    rnd = random.Random(seed)
    coefs = [[rnd.randrange(1, R) for _ in range(t)] for _ in range(n_groups)]
    shares = [[poly_eval(c, x) for x in range(1, n + 1)] for c in coefs]
    return coefs, pack([list(range(1, n + 1))] * n_groups), commitments(eng, coefs), shares


# ---------------------------------------------------------------- 1. ragged groups
def test_ragged_groups(eng):
    rnd = random.Random(1)
    coefs = [[rnd.randrange(1, R) for _ in range(t)] for t in SIZES_T]
    ids = [[rnd.randrange(1, R) for _ in range(n)] for n in SIZES_N]
    shares = [[poly_eval(c, x) for x in xs] for c, xs in zip(coefs, ids)]
    shares[5] = [rnd.randrange(1, R) for _ in range(SIZES_N[5])]      # T = 0: the zero polynomial, and no share of these is zero
    commits = commitments(eng, coefs)
    n = sum(SIZES_N)
    s0, d0 = eng.threshold_key_check_stats(), eng.threshold_deal_stats()
    bm, st = eng.threshold_verify_key_shares_batch(commits, pack(ids), pack(shares))
    s1, d1 = eng.threshold_key_check_stats(), eng.threshold_deal_stats()
    assert st == bytes(len(SIZES_N))
    want = [t > 0 for t, m in zip(SIZES_T, SIZES_N) for _ in range(m)]
    assert bm == synth.bitmap_of(want)
    assert s1["launches"] - s0["launches"] == 1 and s1["shares"] - s0["shares"] == n and s1["table_builds"] == 1
    assert s1["window_bits"] in (4, 8)
    assert d1["g2_launches"] - d0["g2_launches"] == 1 and d1["g2_shares"] - d0["g2_shares"] == n     # the evaluation goes on counting
    comp, cst = composition(eng, commits, pack(ids), pack(shares))
    assert cst == st and comp == want
    # offsets that do not start at 0: groups 2 .. 6 of the same arrays
    ca = np.frombuffer(b"".join(commits), dtype=np.uint8); ia = np.frombuffer(b"".join(pack(ids)), dtype=np.uint8)
    sa = np.frombuffer(b"".join(pack(shares)), dtype=np.uint8)
    coff = np.cumsum([0] + SIZES_T).astype(np.uint64)[2:8]; goff = np.cumsum([0] + SIZES_N).astype(np.uint64)[2:8]
    m = int(goff[-1] - goff[0])
    o = np.full((m + 7) // 8, 0x5a, dtype=np.uint8); s = np.full(5, 0x5a, dtype=np.uint8)
    rc = eng._lib.blsbn254_threshold_verify_key_shares_batch(eng._ctx, ca.ctypes.data_as(u8), coff.ctypes.data_as(u64), ia.ctypes.data_as(u8), sa.ctypes.data_as(u8),
                                                             goff.ctypes.data_as(u64), ctypes.c_size_t(5), o.ctypes.data_as(u8), s.ctypes.data_as(u8))
    assert rc == 0 and s.tobytes() == bytes(5)
    assert o.tobytes() == synth.bitmap_of(want[int(goff[0]):int(goff[-1])])


# ---------------------------------------------------------------- 2. wrong shares, in groups of small ids
def test_wrong_shares_clear_their_own_bit(eng):
    ng, n = 8, 7
    coefs, id_sets, commits, honest = small_groups(eng, ng, 2)
    shares = [list(s) for s in honest]
    want = [True] * (ng * n)

    def spoil(g, i, v):
        assert v != honest[g][i]
        shares[g][i] = v; want[n * g + i] = False

    spoil(0, 0, (honest[0][0] + 1) % R)
    spoil(1, 6, R - honest[1][6])
    spoil(2, 3, honest[2][4])                                         # the neighbour's share
    assert honest[3][2] + R < 1 << 256
    spoil(3, 2, honest[3][2] + R)                                     # the same point, not canonical
    spoil(4, 5, R)
    assert honest[5][1] != 0
    spoil(5, 1, 0)
    spoil(7, 6, (honest[7][6] + 1) % R); spoil(7, 0, R - honest[7][0])   # two in one group, first and last
    bm, st = eng.threshold_verify_key_shares_batch(commits, id_sets, pack(shares))
    assert st == bytes(ng)
    assert bits_of(bm, ng * n) == want and bm == synth.bitmap_of(want)
    assert composition(eng, commits[:3], id_sets[:3], pack(shares[:3]))[0] == want[:3 * n]


def test_zero_share_and_the_empty_polynomial(eng):
    rnd = random.Random(3)
    n, root = 7, 4
    q = [rnd.randrange(1, R) for _ in range(4)]
    f = [(-root * q[0]) % R] + [(q[j - 1] - root * q[j]) % R for j in range(1, 4)] + [q[3]]     # (x - root) q(x)
    assert poly_eval(f, root) == 0 and all(poly_eval(f, x) for x in range(1, n + 1) if x != root)
    ids = pack([list(range(1, n + 1))])[0]
    commits = commitments(eng, [f])
    id_sets, commit_sets = [ids, ids, b32(1) + b32(2) + b32(3)], [commits[0], commits[0], b""]
    share_sets = pack([[0] * n, [poly_eval(f, x) for x in range(1, n + 1)], [0, 5, 0]])
    bm, st = eng.threshold_verify_key_shares_batch(commit_sets, id_sets, share_sets)
    assert st == bytes(3)
    want = [x == root for x in range(1, n + 1)] + [True] * n + [True, False, True]
    assert bits_of(bm, len(want)) == want and bm == synth.bitmap_of(want)


# ---------------------------------------------------------------- 3. bad groups stay local
def test_bad_groups_stay_local(eng):
    ng, n = 8, 7
    coefs, id_sets, commits, honest = small_groups(eng, ng, 4)
    shares = [list(s) for s in honest]
    shares[4][3] = (shares[4][3] + 1) % R                               # a wrong share beside the bad groups
    bad_ids = [list(range(1, n + 1)) for _ in range(ng)]
    bad_c = list(commits)
    bad_ids[0][2] = 0                                                 # id == 0
    bad_ids[1][6] = R + 3                                             # id >= r
    oc = bytearray(commits[2]); oc[128 + 127] ^= 1
    bad_c[2] = bytes(oc)                                              # off the curve (a flipped y byte)
    bad_c[3] = commits[3][:256] + synth.NON_SUBGROUP_PK + commits[3][384:]   # outside the subgroup
    bad_ids[6][0] = R; bad_c[6] = b"\xff" * 128 + commits[6][128:]      # both: the scalar error wins
    bad = {0: ERR_SCALAR, 1: ERR_SCALAR, 2: ERR_G2, 3: ERR_G2, 6: ERR_SCALAR}
    bm, st = eng.threshold_verify_key_shares_batch(bad_c, pack(bad_ids), pack(shares))
    _, st_eval = eng.g2_poly_eval_batch(bad_c, pack(bad_ids))
    assert st == st_eval and list(st) == [bad.get(g, 0) for g in range(ng)]
    want = [g not in bad and not (g == 4 and i == 3) for g in range(ng) for i in range(n)]
    assert bm == synth.bitmap_of(want)
    # without the bad groups the others' bits are the same
    good, gst = eng.threshold_verify_key_shares_batch(commits, id_sets, pack(shares))
    assert gst == bytes(ng)
    assert bits_of(good, ng * n) == [not (g == 4 and i == 3) for g in range(ng) for i in range(n)]


# ---------------------------------------------------------------- 4. launches that end inside groups
def test_launch_boundaries(eng, M, monkeypatch):
    ng, n = 2048, 7
    coefs, id_sets, commits, honest = small_groups(eng, ng, 5)
    shares = [list(s) for s in honest]
    want = [True] * (ng * n)
    for g in range(0, ng, 16):
        i = (g // 16) % n
        shares[g][i] = (shares[g][i] + 1 + g) % R
        want[n * g + i] = False
    share_sets = pack(shares)
    bm, st = eng.threshold_verify_key_shares_batch(commits, id_sets, share_sets)
    assert st == bytes(ng) and bm == synth.bitmap_of(want)
    with monkeypatch.context() as mp:                                # 4104 is no multiple of 7: no launch ends on a group boundary
        mp.setenv("BLSBN254_CHUNK_LANES", "4104")
        e2 = M.Engine(0)
        try:
            bm2, st2 = e2.threshold_verify_key_shares_batch(commits, id_sets, share_sets)
            s = e2.threshold_key_check_stats()
        finally:
            e2.close()
    assert (bm2, st2) == (bm, st)
    chunks = -(-ng * n // 4104)
    assert chunks == 4 and s["launches"] == chunks and s["shares"] == ng * n and s["table_builds"] == 1


# ---------------------------------------------------------------- 5. the life of the table
def test_life_of_the_table(eng, M, oracle):
    dst = M.DEFAULT_DST
    ng, n, t = 8, 5, 3
    coefs, id_sets, commits, honest = small_groups(eng, ng, 6, n=n, t=t)
    shares = [list(s) for s in honest]
    shares[2][1] = (shares[2][1] + 1) % R
    share_sets = pack(shares)
    msgs = [b"table %d" % g for g in range(ng)]
    sigs = eng.sign_batch(b"".join(pack(honest)), [m for m in msgs for _ in range(n)], dst)
    sig_sets = [sigs[64 * n * g:64 * n * (g + 1)] for g in range(ng)]
    vb = synth.make_batch_gpu(eng, oracle, 64, dst, pool=8, invalid_every=7, spot=2)
    e0 = M.Engine(0)
    try:
        fresh = e0.threshold_verify_key_shares_batch(commits, id_sets, share_sets)      # a context that has made no other call
    finally:
        e0.close()
    assert fresh == eng.threshold_verify_key_shares_batch(commits, id_sets, share_sets)
    assert fresh == (synth.bitmap_of([not (g == 2 and i == 1) for g in range(ng) for i in range(n)]), bytes(ng))
    e = M.Engine(0)
    try:
        assert e.threshold_key_check_stats()["table_builds"] == 0
        assert e.threshold_verify_key_shares_batch([b""], [b""], [b""]) == (b"", bytes(1))       # no share: no table yet
        assert e.threshold_key_check_stats()["table_builds"] == 0
        assert e.threshold_verify_key_shares_batch(commits, id_sets, share_sets) == fresh
        assert e.threshold_key_check_stats()["table_builds"] == 1
        assert e.threshold_verify_key_shares_batch(commits, id_sets, share_sets) == fresh
        assert e.threshold_key_check_stats()["table_builds"] == 1
        assert e.g2_poly_eval_batch(commits, id_sets)[1] == bytes(ng)
        assert e.verify_batch(vb[0], vb[1], vb[2], dst) == synth.bitmap_of(vb[3])
        out, used, cst = e.threshold_combine_checked_batch(commits, id_sets, sig_sets, msgs, dst)
        assert cst == bytes(ng)
        assert e.threshold_verify_key_shares_batch(commits, id_sets, share_sets) == fresh
        s = e.threshold_key_check_stats()
        assert s["table_builds"] == 1 and s["launches"] == 3 and s["shares"] == 3 * ng * n
    finally:
        e.close()


# ---------------------------------------------------------------- 6. argument errors
def test_argument_errors(eng):
    lib, ctx = eng._lib, eng._ctx
    coefs = [[3, 4], [5, 6]]
    commits = np.frombuffer(b"".join(commitments(eng, coefs)), dtype=np.uint8)
    ids = np.frombuffer(b"".join(pack([[1, 2], [1, 2]])), dtype=np.uint8)
    shares = np.frombuffer(b"".join(pack([[7, 11], [11, 17]])), dtype=np.uint8)
    out = np.full(1, 0x5a, dtype=np.uint8); st = np.full(2, 0x5a, dtype=np.uint8)
    P = lambda a: a.ctypes.data_as(u8)
    keep = []

    def off(o):
        if o is None:
            return None
        a = np.ascontiguousarray(np.asarray(o, dtype=np.uint64)); keep.append(a)
        return a.ctypes.data_as(u64)

    def kc(coff=(0, 2, 4), goff=(0, 2, 4), n=2, c=ctx, a=P(commits), i=P(ids), s=P(shares), o=P(out), t=P(st)):
        return lib.blsbn254_threshold_verify_key_shares_batch(c, a, off(coff), i, s, off(goff), ctypes.c_size_t(n), o, t)

    def untouched():
        return out.tobytes() == b"\x5a" and st.tobytes() == b"\x5a\x5a"

    errors = [dict(c=None), dict(a=None), dict(coff=None), dict(i=None), dict(s=None), dict(goff=None), dict(o=None), dict(t=None),
              dict(coff=(0, 3, 1)), dict(goff=(0, 3, 1)),                                     # decreasing offsets
              dict(goff=(0, 1, (1 << 23) + 1)), dict(coff=(0, 1, (1 << 23) + 1))]               # more than 2^23 ids / coefficients
    for kw in errors:
        assert kc(**kw) == E_ARG, kw
        assert untouched(), kw
    many = np.zeros((1 << 23) + 2, dtype=np.uint64)                                           # more than 2^23 groups (all empty)
    pm = many.ctypes.data_as(u64)
    assert lib.blsbn254_threshold_verify_key_shares_batch(ctx, None, pm, None, None, pm, ctypes.c_size_t((1 << 23) + 1), P(out), P(st)) == E_ARG
    assert untouched()
    assert kc(n=0) == 0 and kc(coff=None, goff=None, n=0, a=None, i=None, s=None, o=None, t=None) == 0 and untouched()
    assert kc() == 0 and out.tobytes() == b"\x0f" and st.tobytes() == bytes(2)                 # 3 + 4 x and 5 + 6 x at 1, 2
    assert kc(coff=(0, 0, 0), a=None) == 0 and out.tobytes() == b"\x00"                       # no commitments at all: nothing to read
    assert kc(goff=(0, 0, 0), i=None, s=None, o=None) == 0                                    # no ids at all
    assert lib.blsbn254_threshold_key_check_stats(ctx, None) == E_ARG and lib.blsbn254_threshold_key_check_stats(None, (ctypes.c_uint64 * 4)()) == E_ARG
    assert eng.threshold_verify_key_shares_batch([], [], []) == (b"", b"")
    with pytest.raises(ValueError):
        eng.threshold_verify_key_shares_batch([bytes(128)], [bytes(32)], [bytes(64)])
    with pytest.raises(ValueError):
        eng.threshold_verify_key_shares_batch([bytes(128)], [bytes(32)], [])
