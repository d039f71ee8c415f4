"""GPU tests (MI355X) of the threshold dealing side over ragged groups (blsbn254_fr_poly_eval_batch / blsbn254_g2_poly_eval_batch /
blsbn254_threshold_verify_shares_batch) and of the Fr operations of blsbn254_field_op_batch: the scalar field against Python
integers, key shares against a Python Horner, public key shares against sk_to_pk of those shares and against the oracle's
g2_mul / g2_add, the bit count a launch loops over, bad groups that stay local, the whole deal -> sign -> check -> combine flow,
the argument errors, and a long-lived context."""
import ctypes
import random

import numpy as np
import pytest

from tests import synth
from tests.gpu_support import eng, M
from tests.helpers import b32, IDENT1, IDENT2, poly_eval

pytestmark = pytest.mark.gpu
R = synth.R
E_ARG = -1
ERR_SCALAR, ERR_G2 = 1, 3
OP_FP_MUL = 0
OP_FR_MUL, OP_FR_SQR, OP_FR_INV, OP_FR_ADD, OP_FR_SUB, OP_FR_NEG = 64, 65, 66, 67, 68, 69
SIZES_N = [1, 2, 0, 7, 63, 64, 65, 257]
SIZES_T = [1, 2, 3, 8, 33, 0, 5, 4]


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


@pytest.fixture(scope="module")
def ragged(eng):
    """the ragged groups of tests 2 and 3: coefficients and ids random in [1, r), their commitments, the shares by Python"""
    rnd = random.Random(1)
    coefs = [[rnd.randrange(1, R) for _ in range(t)] for t in SIZES_T]
    ids = [[rnd.randrange(1, R) for _ in range(n)] for n in SIZES_N]
    want = b"".join(b32(poly_eval(c, x)) for c, xs in zip(coefs, ids) for x in xs)
    return coefs, ids, commitments(eng, coefs), want


# ---------------------------------------------------------------- 1. Fr operations against Python integers
def test_fr_operations_match_python_integers(eng, M):
    rnd = random.Random(11)
    n = 1003
    xs = [rnd.randrange(R) for _ in range(1000)] + [0, 1, R - 1]
    ys = [rnd.randrange(R) for _ in range(1000)] + [R - 1, 0, R - 1]
    a, b = b"".join(map(b32, xs)), b"".join(map(b32, ys))
    fp_before = eng.field_op_batch(OP_FP_MUL, a, b, n)
    want = {OP_FR_MUL: [x * y % R for x, y in zip(xs, ys)], OP_FR_SQR: [x * x % R for x in xs],
            OP_FR_INV: [pow(x, -1, R) if x else 0 for x in xs], OP_FR_ADD: [(x + y) % R for x, y in zip(xs, ys)],
            OP_FR_SUB: [(x - y) % R for x, y in zip(xs, ys)], OP_FR_NEG: [(-x) % R for x in xs]}
    got = {}
    for op, w in want.items():
        got[op] = eng.field_op_batch(op, a, b if op in eng.FIELD_OP_BINARY else None, n)
        assert got[op] == b"".join(map(b32, w)), op
    assert got[OP_FR_INV][32 * 1000:32 * 1001] == bytes(32)                                    # INV(0) == 0
    prod = eng.field_op_batch(OP_FR_MUL, a, got[OP_FR_INV], n)
    assert prod == b"".join(b32(1 if x else 0) for x in xs)                                   # MUL(a, INV(a)) == 1
    for op in want:                                                                           # an operand equal to r
        bad = a[:32 * 5] + b32(R) + a[32 * 6:]
        with pytest.raises(M.InvalidScalarBytes):
            eng.field_op_batch(op, bad, b if op in eng.FIELD_OP_BINARY else None, n)
    with pytest.raises(M.InvalidScalarBytes):
        eng.field_op_batch(OP_FR_ADD, a, b[:-32] + b32(R), n)
    with pytest.raises(M.InvalidGtBytes):                                                     # the tower operations keep their code
        eng.field_op_batch(OP_FP_MUL, b32(synth.P) + a[32:], b, n)
    assert eng.field_op_batch(OP_FP_MUL, a, b, n) == fp_before
    P = synth.P
    assert fp_before[:32 * 8] == b"".join(b32(x * y % P) for x, y in zip(xs[:8], ys[:8]))


# ---------------------------------------------------------------- 2. ragged Fr evaluation
def test_ragged_fr_evaluation(eng, ragged):
    coefs, ids, _, want = ragged
    s0 = eng.threshold_deal_stats()
    out, st = eng.fr_poly_eval_batch(pack(coefs), pack(ids))
    s1 = eng.threshold_deal_stats()
    assert st == bytes(len(SIZES_N)) and out == want
    assert s1["fr_shares"] - s0["fr_shares"] == sum(SIZES_N) and s1["g2_shares"] == s0["g2_shares"]
    pos = sum(SIZES_N[:5])
    assert out[32 * pos:32 * (pos + 64)] == bytes(32 * 64)                                    # t = 0: the zero polynomial
    # offsets that do not start at 0: groups 3 .. 6 of the same arrays
    u8 = ctypes.POINTER(ctypes.c_uint8); u64 = ctypes.POINTER(ctypes.c_uint64)
    ca = np.frombuffer(b"".join(pack(coefs)), dtype=np.uint8); ia = np.frombuffer(b"".join(pack(ids)), dtype=np.uint8)
    coff = np.cumsum([0] + SIZES_T).astype(np.uint64)[3:8]; goff = np.cumsum([0] + SIZES_N).astype(np.uint64)[3:8]
    n = int(goff[-1] - goff[0])
    o = np.zeros(32 * n, dtype=np.uint8); s = np.full(4, 0x5a, dtype=np.uint8)
    rc = eng._lib.blsbn254_fr_poly_eval_batch(eng._ctx, ca.ctypes.data_as(u8), coff.ctypes.data_as(u64), ia.ctypes.data_as(u8), goff.ctypes.data_as(u64),
                                              ctypes.c_size_t(4), o.ctypes.data_as(u8), s.ctypes.data_as(u8))
    assert rc == 0 and s.tobytes() == bytes(4)
    assert o.tobytes() == want[32 * int(goff[0]):32 * int(goff[-1])]


# ---------------------------------------------------------------- 3. ragged G2 evaluation
def test_ragged_g2_evaluation(eng, oracle, ragged):
    coefs, ids, commits, want = ragged
    n = sum(SIZES_N)
    s0 = eng.threshold_deal_stats()
    pks, st = eng.g2_poly_eval_batch(commits, pack(ids))
    s1 = eng.threshold_deal_stats()
    assert st == bytes(len(SIZES_N))
    assert s1["g2_shares"] - s0["g2_shares"] == n and s1["g2_launches"] - s0["g2_launches"] == 1 and s1["id_bits"] == 254
    shares, _ = eng.fr_poly_eval_batch(pack(coefs), pack(ids))
    assert shares == want
    # (sk_to_pk rejects nothing here: a share is 0 with probability 2^-254; the t = 0 group's shares ARE 0 and give the identity)
    assert pks == eng.sk_to_pk_batch(shares, n)
    pos = sum(SIZES_N[:5])
    assert pks[128 * pos:128 * (pos + 64)] == IDENT2 * 64
    rnd = random.Random(3)
    starts = np.cumsum([0] + SIZES_N)
    picks = [(g, i) for g in (0, 1, 3, 4, 6, 7) for i in sorted(rnd.sample(range(SIZES_N[g]), min(2, SIZES_N[g])))][:12]
    picks += [(7, 256)] * (12 - len(picks))
    assert len(picks) == 12
    for g, i in picks:
        cm = [commits[g][128 * j:128 * j + 128] for j in range(SIZES_T[g])]
        acc = cm[-1]
        for c in reversed(cm[:-1]):
            acc = oracle.g2_add(oracle.g2_mul(acc, ids[g][i]), c)
        p = int(starts[g]) + i
        assert pks[128 * p:128 * p + 128] == acc, (g, i)
    # offsets that do not start at 0
    u8 = ctypes.POINTER(ctypes.c_uint8); u64 = ctypes.POINTER(ctypes.c_uint64)
    ca = np.frombuffer(b"".join(commits), dtype=np.uint8); ia = np.frombuffer(b"".join(pack(ids)), dtype=np.uint8)
    coff = np.cumsum([0] + SIZES_T).astype(np.uint64)[2:6]; goff = starts.astype(np.uint64)[2:6]
    m = int(goff[-1] - goff[0])
    o = np.zeros(128 * m, dtype=np.uint8); s = np.full(3, 0x5a, dtype=np.uint8)
    rc = eng._lib.blsbn254_g2_poly_eval_batch(eng._ctx, ca.ctypes.data_as(u8), coff.ctypes.data_as(u64), ia.ctypes.data_as(u8), goff.ctypes.data_as(u64),
                                              ctypes.c_size_t(3), o.ctypes.data_as(u8), s.ctypes.data_as(u8))
    assert rc == 0 and s.tobytes() == bytes(3) and o.tobytes() == pks[128 * int(goff[0]):128 * int(goff[-1])]


# ---------------------------------------------------------------- 4. the bit count of a launch
def test_bit_count(eng):
    rnd = random.Random(4)
    coefs = [[rnd.randrange(1, R) for _ in range(3)] for _ in range(5)]
    commits = commitments(eng, coefs)
    small = [list(range(1, 8))] * 4
    pks, st = eng.g2_poly_eval_batch(commits[:4], pack(small))
    assert st == bytes(4) and eng.threshold_deal_stats()["id_bits"] == 3
    shares = b"".join(b32(poly_eval(c, x)) for c, xs in zip(coefs, small) for x in xs)
    assert pks == eng.sk_to_pk_batch(shares, 28)
    for extra, bits, ok in (((1 << 64) + 1, 65, True), (R - 1, 254, True), (R, 254, False), ((1 << 255) + 5, 254, False)):
        got, st = eng.g2_poly_eval_batch(commits, pack(small + [[extra]]))
        nb = eng.threshold_deal_stats()["id_bits"]
        assert nb == bits if ok else 3 <= nb <= 254, (hex(extra), nb)
        assert got[:128 * 28] == pks, hex(extra)                                              # the first groups' bytes are unchanged
        if ok:
            assert st == bytes(5) and got[128 * 28:] == eng.sk_to_pk_batch(b32(poly_eval(coefs[4], extra)), 1)
        else:
            assert st == bytes(4) + bytes([ERR_SCALAR]) and got[128 * 28:] == IDENT2


# ---------------------------------------------------------------- 5. bad inputs stay local
def test_bad_inputs_stay_local(eng, oracle):
    rnd = random.Random(5)
    coefs = [[rnd.randrange(1, R) for _ in range(3)] for _ in range(8)]
    ids = [rnd.sample(range(1, 1000), 5) for _ in range(8)]
    ids[6][4] = ids[6][0]                                                                     # a repeated id is accepted
    commits = commitments(eng, coefs)
    good, gst = eng.g2_poly_eval_batch(commits, pack(ids))
    assert gst == bytes(8)
    shares = b"".join(b32(poly_eval(c, x)) for c, xs in zip(coefs, ids) for x in xs)
    assert good == eng.sk_to_pk_batch(shares, 40)
    assert good[128 * 30:128 * 31] == good[128 * 34:128 * 35] == oracle.sk_to_pk(poly_eval(coefs[6], ids[6][0]))
    bad_ids, bad_c = [list(x) for x in ids], list(commits)
    bad_ids[0][2] = R + 3                                                                     # id >= r
    bad_ids[1][0] = 0                                                                         # id == 0
    oc = bytearray(commits[2]); oc[128 + 127] ^= 1
    bad_c[2] = bytes(oc)                                                                      # off the curve (a flipped y byte)
    bad_c[3] = commits[3][:256] + synth.NON_SUBGROUP_PK                                       # outside the subgroup
    bad_ids[5][4] = R; bad_c[5] = b"\xff" * 128 + commits[5][128:]                            # both: the scalar error wins
    want = {0: ERR_SCALAR, 1: ERR_SCALAR, 2: ERR_G2, 3: ERR_G2, 5: ERR_SCALAR}
    out, st = eng.g2_poly_eval_batch(bad_c, pack(bad_ids))
    assert list(st) == [want.get(g, 0) for g in range(8)]
    for g in range(8):
        assert out[640 * g:640 * (g + 1)] == (IDENT2 * 5 if g in want else good[640 * g:640 * (g + 1)]), g
    # the same on the scalar side: a coefficient >= r, an id >= r, an id 0
    bad_f = [list(c) for c in coefs]
    bad_f[4][1] = R
    fout, fst = eng.fr_poly_eval_batch(pack(bad_f), pack(bad_ids))
    assert list(fst) == [ERR_SCALAR if g in (0, 1, 4, 5) else 0 for g in range(8)]
    for g in range(8):
        assert fout[160 * g:160 * (g + 1)] == (bytes(160) if g in (0, 1, 4, 5) else shares[160 * g:160 * (g + 1)]), g
    # and in the check of partial signatures: every bit of a bad group is 0, the others as without the bad groups
    msgs = [b"group %d" % g for g in range(8)]
    sigs = eng.sign_batch(shares, [m for m in msgs for _ in range(5)], b"TEST-DST")
    sig_sets = [sigs[320 * g:320 * (g + 1)] for g in range(8)]
    bm, st2 = eng.threshold_verify_shares_batch(bad_c, pack(bad_ids), sig_sets, msgs, b"TEST-DST")
    assert list(st2) == list(st)
    assert bm == synth.bitmap_of([g not in want for g in range(8) for _ in range(5)])


# ---------------------------------------------------------------- 6. the whole flow
def _flow(eng, oracle, n_groups, bad_every, seed, dst):
    """n_groups x (n = 5, t = 3, ids 1 .. 5), one message per group; group g with g % bad_every == 0 holds ONE bad share, of
    the kind (g // bad_every) % 3.  Returns what the checks below need."""
    rnd = random.Random(seed)
    n, t = 5, 3
    coefs = [[rnd.randrange(1, R) for _ in range(t)] for _ in range(n_groups)]
    id_sets = pack([list(range(1, n + 1))] * n_groups)
    commits = commitments(eng, coefs)
    msgs = [b"deal message %d" % g for g in range(n_groups)]
    shares, st = eng.fr_poly_eval_batch(pack(coefs), id_sets)
    assert st == bytes(n_groups)
    for g in (0, n_groups // 2, n_groups - 1):
        assert shares[160 * g:160 * (g + 1)] == b"".join(b32(poly_eval(coefs[g], x)) for x in range(1, n + 1))
    sk = bytearray(shares)
    per_share_msgs = [m for m in msgs for _ in range(n)]
    expect = [True] * (n * n_groups)
    ident = []
    for g in range(0, n_groups, bad_every):
        kind, i = (g // bad_every) % 3, n * g + (g // bad_every) % n
        expect[i] = False
        if kind == 0:
            per_share_msgs[i] = msgs[(g + 1) % n_groups]             # signed over another group's message
        elif kind == 1:
            j = i + 1 if i % n < n - 1 else i - 1
            sk[32 * i:32 * i + 32] = shares[32 * j:32 * j + 32]      # signed with a neighbour's share key
        else:
            ident.append(i)                                          # replaced by the identity encoding
    sigs = bytearray(eng.sign_batch(bytes(sk), per_share_msgs, dst))
    for i in ident:
        sigs[64 * i:64 * i + 64] = IDENT1
    sigs = bytes(sigs)
    i = n + 2                                                        # group 1 (never a bad one), id 3
    assert expect[i] and sigs[64 * i:64 * i + 64] == oracle.sign(poly_eval(coefs[1], 3), msgs[1], dst)
    sig_sets = [sigs[64 * n * g:64 * n * (g + 1)] for g in range(n_groups)]
    return coefs, id_sets, commits, msgs, sigs, sig_sets, expect


def _check_flow(e, M, flow, n_groups, dst, combine):
    coefs, id_sets, commits, msgs, sigs, sig_sets, expect = flow
    n = 5
    bm, st = e.threshold_verify_shares_batch(commits, id_sets, sig_sets, msgs, dst)
    assert st == bytes(n_groups)
    assert bm == synth.bitmap_of(expect)
    if not combine:
        return bm
    pks, st = e.g2_poly_eval_batch(commits, id_sets)
    assert st == bytes(n_groups)
    assert bm == e.verify_batch(pks, [m for m in msgs for _ in range(n)], sigs, dst)
    # interpolate over three shares per group whose bits are set: the result verifies under C_0
    ids3, sigs3 = [], []
    for g in range(n_groups):
        live = [i for i in range(n) if expect[n * g + i]][:3]
        assert len(live) == 3
        ids3.append(b"".join(b32(i + 1) for i in live))
        sigs3.append(b"".join(sig_sets[g][64 * i:64 * i + 64] for i in live))
    out, cst = e.threshold_combine_batch(ids3, sigs3)
    assert cst == bytes(n_groups)
    c0 = b"".join(c[:128] for c in commits)
    assert e.verify_batch(c0, msgs, out, dst) == synth.bitmap_of([True] * n_groups)
    return bm


def test_the_whole_flow(eng, oracle, M):
    dst = M.DEFAULT_DST
    flow = _flow(eng, oracle, 64, 4, 6, dst)
    assert flow[6].count(False) == 16
    _check_flow(eng, M, flow, 64, dst, True)


def test_the_whole_flow_over_several_launches(eng, oracle, M, monkeypatch):
    dst = M.DEFAULT_DST
    ng = 1 << 12
    flow = _flow(eng, oracle, ng, 16, 7, dst)
    s0 = eng.threshold_deal_stats()
    bm = _check_flow(eng, M, flow, ng, dst, True)
    s1 = eng.threshold_deal_stats()
    assert s1["g2_launches"] - s0["g2_launches"] == 2 and s1["id_bits"] == 3
    with monkeypatch.context() as mp:                                # more than one launch chunk, none ending on a group boundary
        mp.setenv("BLSBN254_CHUNK_LANES", "4104")
        e2 = M.Engine(0)
        try:
            assert _check_flow(e2, M, flow, ng, dst, False) == bm
            assert e2.threshold_deal_stats()["g2_launches"] == 5
            pks2, _ = e2.g2_poly_eval_batch(flow[2], flow[1])
            sh2, _ = e2.fr_poly_eval_batch(pack(flow[0]), flow[1])
        finally:
            e2.close()
    assert (pks2, bytes(ng)) == eng.g2_poly_eval_batch(flow[2], flow[1])
    assert pks2 == eng.sk_to_pk_batch(sh2, 5 * ng)


# ---------------------------------------------------------------- 7. argument errors
def test_argument_errors(eng):
    lib, ctx = eng._lib, eng._ctx
    u8 = ctypes.POINTER(ctypes.c_uint8); u64 = ctypes.POINTER(ctypes.c_uint64)
    coefs = [[3, 4], [5, 6]]
    commits = np.frombuffer(b"".join(commitments(eng, coefs)), dtype=np.uint8)
    cf = np.frombuffer(b"".join(pack(coefs)), dtype=np.uint8)
    ids = np.frombuffer(b"".join(pack([[1, 2], [1, 2]])), dtype=np.uint8)
    sigs = np.frombuffer(IDENT1 * 4, dtype=np.uint8)
    msgs = np.frombuffer(b"abcd", dtype=np.uint8)
    out = np.zeros(128 * 4, dtype=np.uint8); st = np.zeros(4, dtype=np.uint8)
    P = lambda a: a.ctypes.data_as(u8)
    keep = []

    def off(o):
        if o is None:
            return None
        a = np.ascontiguousarray(np.asarray(o, dtype=np.uint64)); keep.append(a)
        return a.ctypes.data_as(u64)

    def fr(coff=(0, 2, 4), goff=(0, 2, 4), n=2, c=ctx, a=P(cf), i=P(ids), o=P(out), t=P(st)):
        return lib.blsbn254_fr_poly_eval_batch(c, a, off(coff), i, off(goff), ctypes.c_size_t(n), o, t)

    def g2(coff=(0, 2, 4), goff=(0, 2, 4), n=2, c=ctx, a=P(commits), i=P(ids), o=P(out), t=P(st)):
        return lib.blsbn254_g2_poly_eval_batch(c, a, off(coff), i, off(goff), ctypes.c_size_t(n), o, t)

    def vs(coff=(0, 2, 4), goff=(0, 2, 4), n=2, c=ctx, a=P(commits), i=P(ids), o=P(out), t=P(st), s=P(sigs), m=P(msgs), moff=(0, 2, 4), d=b"TEST", dl=4):
        return lib.blsbn254_threshold_verify_shares_batch(c, a, off(coff), i, s, off(goff), m, off(moff), ctypes.c_size_t(n), d, ctypes.c_size_t(dl), o, t)

    for fn in (fr, g2, vs):
        assert fn() == 0
        assert fn(coff=(0, 3, 1)) == E_ARG and fn(goff=(0, 3, 1)) == E_ARG                   # decreasing offsets
        assert fn(goff=(0, 1, (1 << 23) + 1)) == E_ARG and fn(coff=(0, 1, (1 << 23) + 1)) == E_ARG
        assert fn(c=None) == E_ARG and fn(a=None) == E_ARG and fn(i=None) == E_ARG and fn(o=None) == E_ARG and fn(t=None) == E_ARG
        assert fn(coff=None) == E_ARG and fn(goff=None) == E_ARG
        assert fn(n=0) == 0 and fn(coff=None, goff=None, n=0, a=None, i=None, o=None, t=None) == 0
        assert fn(coff=(0, 0, 0), a=None) == 0                                               # no coefficients at all: nothing to read
    assert vs(moff=(0, 3, 1)) == E_ARG and vs(moff=None) == E_ARG and vs(s=None) == E_ARG and vs(d=None) == E_ARG
    assert vs(m=None) == E_ARG and vs(m=None, moff=(0, 0, 0)) == 0 and vs(d=None, dl=0) == 0
    assert lib.blsbn254_threshold_deal_stats(ctx, None) == E_ARG and lib.blsbn254_threshold_deal_stats(None, (ctypes.c_uint64 * 4)()) == E_ARG
    assert eng.fr_poly_eval_batch([], []) == (b"", b"") and eng.g2_poly_eval_batch([], []) == (b"", b"")
    assert eng.threshold_verify_shares_batch([], [], [], [], b"TEST") == (b"", b"")
    with pytest.raises(ValueError):
        eng.g2_poly_eval_batch([bytes(128)], [])
    with pytest.raises(ValueError):
        eng.fr_poly_eval_batch([bytes(33)], [bytes(32)])
    with pytest.raises(ValueError):
        eng.threshold_verify_shares_batch([bytes(128)], [bytes(32)], [bytes(128)], [b""], b"TEST")


# ---------------------------------------------------------------- 8. on a long-lived context
def test_on_a_long_lived_context(M, eng, oracle):
    dst = M.DEFAULT_DST
    rnd = random.Random(9)
    vb = synth.make_batch_gpu(eng, oracle, 1200, dst, pool=40, invalid_every=7, spot=4)        # repeated keys: the prepared path
    flow = _flow(eng, oracle, 96, 8, 10, dst)
    coefs, id_sets, commits, msgs, sigs, sig_sets, expect = flow
    ids3 = [b32(1) + b32(3) + b32(5)] * 96
    sigs3 = [s[:64] + s[128:192] + s[256:320] for s in sig_sets]
    seed = bytes(range(32))
    new = {1, 3}
    steps = [
        lambda e: e.verify_batch(vb[0], vb[1], vb[2], dst),
        lambda e: e.threshold_verify_shares_batch(commits, id_sets, sig_sets, msgs, dst),
        lambda e: e.verify_batch_rlc(vb[0], vb[1], vb[2], dst, seed=seed),
        lambda e: e.g2_poly_eval_batch(commits, id_sets),
        lambda e: e.threshold_combine_batch(ids3, sigs3),
    ]
    fresh = []
    for f in steps:
        e = M.Engine(0)
        try:
            fresh.append(f(e))
        finally:
            e.close()
    assert fresh[0] == fresh[2] == synth.bitmap_of(vb[3])
    assert fresh[1] == (synth.bitmap_of(expect), bytes(96))
    e = M.Engine(0)
    try:
        got = [f(e) for f in steps]
        assert e.path_stats()[0] >= 1
    finally:
        e.close()
    e = M.Engine(0)
    try:
        without = {k: f(e) for k, f in enumerate(steps) if k not in new}
    finally:
        e.close()
    for k, (a, b) in enumerate(zip(got, fresh)):
        assert a == b, "step %d differs from the same call on a context of its own" % k
    for k, b in without.items():
        assert got[k] == b, "step %d differs from the sequence without the new calls" % k
