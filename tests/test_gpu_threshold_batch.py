"""GPU tests (MI355X) of the threshold combine over ragged groups of partial signatures (blsbn254_threshold_combine_batch /
blsbn254_lagrange_at_zero_batch): every group against the oracle and against the single-group call on the same context, the
closed form sigma = [f(0)] H(m) at scale with the BLS verification of the outputs, bad groups that stay local, the edges, both
sides of the hand-over to the single-group pipeline and of a launch chunk, the argument errors, and a long-lived context."""
import ctypes
import random

import numpy as np
import pytest

from tests import synth
from tests.gpu_support import eng, M
from tests.helpers import b32, IDENT1, poly_eval

pytestmark = pytest.mark.gpu
R = synth.R
E_ARG = -1
ERR_SCALAR, ERR_G1 = 1, 2


def random_groups(eng, oracle, rnd, sizes):
    """ids random in [1, r), partial signatures random multiples of a hash (made on the GPU, first and last against the oracle)"""
    n = sum(sizes)
    H = oracle.hash_to_g1_batch([b"threshold batch"], b"TEST-DST")
    ks = [rnd.randrange(1, R) for _ in range(n)]
    pts = eng.g1_mul_batch(H * n, b"".join(map(b32, ks)), n) if n else b""
    for i in ((0, n - 1) if n else ()):
        assert pts[64 * i:64 * i + 64] == oracle.g1_mul(H, ks[i])
    id_sets, sig_sets, pos = [], [], 0
    for t in sizes:
        id_sets.append(b"".join(b32(rnd.randrange(1, R)) for _ in range(t)))
        sig_sets.append(pts[64 * pos:64 * (pos + t)])
        pos += t
    return id_sets, sig_sets


def closed_form_groups(eng, oracle, rnd, sizes, dst, pool_extra=3, spot=16):
    """Group g: a polynomial f_g of degree min(t_g, 33) - 1 (any t_g > deg f_g points interpolate f_g(0); a group of 7 has
    degree 6), a message m_g, t_g ids drawn from 1 .. t_g + pool_extra; shares [f_g(x_i)] H(m_g) made by sign_batch (`spot` of
    them against the oracle).  Returns (id_sets, sig_sets, secrets, msgs)."""
    id_sets, sks, msgs_per_share, secrets, msgs = [], [], [], [], []
    for g, t in enumerate(sizes):
        coeffs = [rnd.randrange(1, R) for _ in range(min(max(t, 1), 33))]
        ids = rnd.sample(range(1, t + pool_extra + 1), t)
        m = b"threshold message %d" % g
        id_sets.append(b"".join(map(b32, ids)))
        sks += [poly_eval(coeffs, x) for x in ids]
        msgs_per_share += [m] * t
        secrets.append(coeffs[0]); msgs.append(m)
    n = len(sks)
    sigs = eng.sign_batch(b"".join(map(b32, sks)), msgs_per_share, dst) if n else b""
    for i in (sorted(rnd.sample(range(n), min(spot, n))) if n else ()):
        assert sigs[64 * i:64 * i + 64] == oracle.g1_mul(oracle.hash_to_g1_batch([msgs_per_share[i]], dst), sks[i])
    sig_sets, pos = [], 0
    for t in sizes:
        sig_sets.append(sigs[64 * pos:64 * (pos + t)])
        pos += t
    return id_sets, sig_sets, secrets, msgs


def check_closed_form(eng, dst, sizes, secrets, msgs, out, status, verify=True):
    """out_g == [f_g(0)] H(m_g) (sign_batch) for every non-empty group, status all 0, and the outputs verify under [f_g(0)] G2"""
    ng = len(sizes)
    assert status == bytes(ng)
    want = eng.sign_batch(b"".join(map(b32, secrets)), msgs, dst)
    for g in range(ng):
        assert out[64 * g:64 * g + 64] == (want[64 * g:64 * g + 64] if sizes[g] else IDENT1), g
    if verify:
        live = [g for g in range(ng) if sizes[g]]
        pks = eng.sk_to_pk_batch(b"".join(b32(secrets[g]) for g in live), len(live))
        bm = eng.verify_batch(pks, [msgs[g] for g in live], b"".join(out[64 * g:64 * g + 64] for g in live), dst)
        assert bm == synth.bitmap_of([True] * len(live))


def single_calls(e, id_sets, sig_sets):
    return b"".join(e.threshold_combine(i, s, len(i) // 32) if i else IDENT1 for i, s in zip(id_sets, sig_sets))


# ---------------------------------------------------------------- 1. oracle parity, ragged
def test_ragged_groups_match_the_oracle(eng, oracle):
    rnd = random.Random(1)
    sizes = [1, 2, 3, 7, 1, 0, 20, 33, 63, 64, 65, 100, 257]
    id_sets, sig_sets = random_groups(eng, oracle, rnd, sizes)
    out, st = eng.threshold_combine_batch(id_sets, sig_sets)
    assert st == bytes(len(sizes))
    for g, t in enumerate(sizes):
        assert out[64 * g:64 * g + 64] == (oracle.threshold_combine(id_sets[g], sig_sets[g], t) if t else IDENT1), g
    lam, st = eng.lagrange_at_zero_batch(id_sets)
    assert st == bytes(len(sizes))
    pos = 0
    for g, t in enumerate(sizes):
        assert lam[32 * pos:32 * (pos + t)] == (oracle.fr_lagrange_at_zero(id_sets[g], t) if t else b""), g
        pos += t


def test_offsets_need_not_start_at_zero(eng, oracle):
    rnd = random.Random(2)
    sizes = [2, 3, 0, 4]
    id_sets, sig_sets = random_groups(eng, oracle, rnd, sizes)
    ids = np.frombuffer(b"".join(id_sets), dtype=np.uint8); sigs = np.frombuffer(b"".join(sig_sets), dtype=np.uint8)
    off = np.array([2, 5, 5, 9], dtype=np.uint64)                   # the first group belongs to no one
    out = np.zeros(64 * 3, dtype=np.uint8); st = np.full(3, 0x5a, dtype=np.uint8); lam = np.zeros(32 * 7, dtype=np.uint8)
    u8 = ctypes.POINTER(ctypes.c_uint8); u64 = ctypes.POINTER(ctypes.c_uint64)
    rc = eng._lib.blsbn254_threshold_combine_batch(eng._ctx, ids.ctypes.data_as(u8), sigs.ctypes.data_as(u8), off.ctypes.data_as(u64), ctypes.c_size_t(3),
                                                   out.ctypes.data_as(u8), st.ctypes.data_as(u8))
    assert rc == 0 and st.tobytes() == bytes(3)
    want = [oracle.threshold_combine(id_sets[g], sig_sets[g], sizes[g]) if sizes[g] else IDENT1 for g in (1, 2, 3)]
    assert out.tobytes() == b"".join(want)
    rc = eng._lib.blsbn254_lagrange_at_zero_batch(eng._ctx, ids.ctypes.data_as(u8), off.ctypes.data_as(u64), ctypes.c_size_t(3), lam.ctypes.data_as(u8), st.ctypes.data_as(u8))
    assert rc == 0 and lam.tobytes() == oracle.fr_lagrange_at_zero(id_sets[1], 3) + oracle.fr_lagrange_at_zero(id_sets[3], 4)


# ---------------------------------------------------------------- 2. equal to the single call
def test_equal_to_the_single_call_before_and_after(eng, oracle):
    rnd = random.Random(3)
    sizes = [7, 1, 0, 33, 5, 100, 2, 64]
    id_sets, sig_sets = random_groups(eng, oracle, rnd, sizes)
    before = single_calls(eng, id_sets, sig_sets)
    out, st = eng.threshold_combine_batch(id_sets, sig_sets)
    after = single_calls(eng, id_sets, sig_sets)
    assert st == bytes(len(sizes)) and out == before == after


# ---------------------------------------------------------------- 3. closed form at scale
@pytest.mark.parametrize("n_groups", [4096, 1 << 16])
def test_closed_form_at_scale(eng, oracle, M, n_groups):
    rnd = random.Random(4 + n_groups)
    dst = M.DEFAULT_DST
    sizes = [7] * n_groups                                           # 7 shares drawn from 10, f_g of degree 6
    id_sets, sig_sets, secrets, msgs = closed_form_groups(eng, oracle, rnd, sizes, dst)
    s0 = eng.threshold_batch_stats()
    out, st = eng.threshold_combine_batch(id_sets, sig_sets)
    s1 = eng.threshold_batch_stats()
    assert s1["batched_groups"] - s0["batched_groups"] == n_groups and s1["single_groups"] == s0["single_groups"]
    check_closed_form(eng, dst, sizes, secrets, msgs, out, st)
    assert out[:64] == oracle.sign(secrets[0], msgs[0], dst)


# ---------------------------------------------------------------- 4. bad groups stay local
def test_bad_groups_stay_local(eng, oracle):
    rnd = random.Random(5)
    sizes = [rnd.randint(2, 9) for _ in range(64)]
    id_sets, sig_sets = random_groups(eng, oracle, rnd, sizes)
    id_sets[40] = id_sets[41][:32 * min(sizes[40], sizes[41])] + id_sets[40][32 * min(sizes[40], sizes[41]):]     # two groups share ids: fine
    sig_sets[50] = IDENT1 + sig_sets[50][64:]                        # an identity partial signature contributes nothing
    good_out, good_st = eng.threshold_combine_batch(id_sets, sig_sets)
    assert good_st == bytes(64)
    for g in (40, 41, 50):
        assert good_out[64 * g:64 * g + 64] == oracle.threshold_combine(id_sets[g], sig_sets[g], sizes[g])
    bad_ids, bad_sigs = list(id_sets), list(sig_sets)
    off_curve = bytearray(sig_sets[33][:64]); off_curve[63] ^= 1
    bad_ids[3] = b32(R) + id_sets[3][32:]                            # id >= r
    bad_ids[10] = id_sets[10][:32] + b32(0) + id_sets[10][64:]       # id == 0
    bad_ids[17] = id_sets[17][:-32] + id_sets[17][:32]               # repeated inside the group
    bad_sigs[25] = sig_sets[25][:64] + b"\xff" * 64 + sig_sets[25][128:]     # does not decode
    bad_sigs[33] = bytes(off_curve) + sig_sets[33][64:]              # off the curve
    bad_ids[47] = b32(R + 5) + id_sets[47][32:]; bad_sigs[47] = sig_sets[47][:-64] + b"\xff" * 64   # both: the scalar error wins
    want = {3: ERR_SCALAR, 10: ERR_SCALAR, 17: ERR_SCALAR, 25: ERR_G1, 33: ERR_G1, 47: ERR_SCALAR}
    out, st = eng.threshold_combine_batch(bad_ids, bad_sigs)
    assert list(st) == [want.get(g, 0) for g in range(64)]
    for g in range(64):
        assert out[64 * g:64 * g + 64] == (IDENT1 if g in want else good_out[64 * g:64 * g + 64]), g
    # the single call's return code for each bad group alone (the off-curve one excepted: the single call does not test that)
    for g, code in want.items():
        if g == 33:
            continue
        buf = (ctypes.c_uint8 * 64)()
        a = np.frombuffer(bad_ids[g], dtype=np.uint8); s = np.frombuffer(bad_sigs[g], dtype=np.uint8)
        u8 = ctypes.POINTER(ctypes.c_uint8)
        assert eng._lib.blsbn254_threshold_combine(eng._ctx, a.ctypes.data_as(u8), s.ctypes.data_as(u8), ctypes.c_size_t(sizes[g]), buf) == code, g
    lam, lst = eng.lagrange_at_zero_batch(bad_ids)
    assert list(lst) == [ERR_SCALAR if want.get(g) == ERR_SCALAR else 0 for g in range(64)]
    pos = 0
    for g, t in enumerate(sizes):
        assert lam[32 * pos:32 * (pos + t)] == (bytes(32 * t) if lst[g] else oracle.fr_lagrange_at_zero(bad_ids[g], t)), g
        pos += t


# ---------------------------------------------------------------- 5. edges
def test_edges(eng, oracle):
    assert eng.threshold_combine_batch([], []) == (b"", b"")
    assert eng.lagrange_at_zero_batch([]) == (b"", b"")
    assert eng.threshold_combine_batch([b""] * 5, [b""] * 5) == (IDENT1 * 5, bytes(5))
    assert eng.lagrange_at_zero_batch([b""] * 5) == (b"", bytes(5))
    rnd = random.Random(6)
    H = oracle.hash_to_g1_batch([b"edge"], b"TEST-DST")
    P = oracle.g1_mul(H, rnd.randrange(1, R))
    # t = 1: lambda = 1, the output is the input point
    # two shares that cancel: sigma_2 = [-lambda_1 / lambda_2] sigma_1
    x1, x2 = rnd.randrange(1, R), rnd.randrange(1, R)
    l1 = x2 * pow(x2 - x1, -1, R) % R; l2 = x1 * pow(x1 - x2, -1, R) % R
    Q = oracle.g1_mul(P, (-l1 * pow(l2, -1, R)) % R)
    out, st = eng.threshold_combine_batch([b32(rnd.randrange(1, R)), b32(x1) + b32(x2), b""], [P, P + Q, b""])
    assert st == bytes(3)
    assert out == P + IDENT1 + IDENT1
    assert oracle.threshold_combine(b32(x1) + b32(x2), P + Q, 2) == IDENT1


# ---------------------------------------------------------------- 6. both sides of the hand-over and of a chunk
def _handover_batch(eng, oracle, M, seed):
    rnd = random.Random(seed)
    T = eng.threshold_batch_stats()["t_big"]
    sizes = [rnd.randint(1, 9) for _ in range(40)]
    sizes[5:5] = [T - 1]; sizes[17:17] = [T + 1]; sizes[30:30] = [T]; sizes[12:12] = [0]
    dst = M.DEFAULT_DST
    id_sets, sig_sets, secrets, msgs = closed_form_groups(eng, oracle, rnd, sizes, dst, spot=8)
    return T, sizes, id_sets, sig_sets, secrets, msgs, dst


def test_both_sides_of_the_hand_over_and_of_a_chunk(M, eng, oracle, monkeypatch):
    T, sizes, id_sets, sig_sets, secrets, msgs, dst = _handover_batch(eng, oracle, M, 7)
    big = [g for g, t in enumerate(sizes) if t > T]
    assert len(big) == 1 and sizes[big[0]] == T + 1
    s0 = eng.threshold_batch_stats()
    out, st = eng.threshold_combine_batch(id_sets, sig_sets)
    s1 = eng.threshold_batch_stats()
    assert s1["single_groups"] - s0["single_groups"] == 1 and s1["batched_groups"] - s0["batched_groups"] == len(sizes) - 1
    assert s1["launches"] - s0["launches"] >= 1
    check_closed_form(eng, dst, sizes, secrets, msgs, out, st)
    assert out == single_calls(eng, id_sets, sig_sets)
    lam, lst = eng.lagrange_at_zero_batch(id_sets)
    assert lst == bytes(len(sizes))
    assert lam == b"".join(eng.lagrange_at_zero(i, len(i) // 32) for i in id_sets)
    for chunk in ("64", "8"):                                        # a chunk smaller than a group: a launch takes a whole group
        with monkeypatch.context() as mp:
            mp.setenv("BLSBN254_CHUNK_LANES", chunk)
            e2 = M.Engine(0)
            try:
                assert e2.threshold_combine_batch(id_sets, sig_sets) == (out, st), chunk
                assert e2.lagrange_at_zero_batch(id_sets) == (lam, lst), chunk
                assert e2.threshold_batch_stats()["launches"] > 2 * (s1["launches"] - s0["launches"])
            finally:
                e2.close()
    # an off-curve share in the group of T + 1 and an id == 0 in the group of T - 1
    gb, gs = big[0], sizes.index(T - 1)
    bad_ids, bad_sigs = list(id_sets), list(sig_sets)
    oc = bytearray(sig_sets[gb]); oc[64 * (T // 2) + 63] ^= 1
    bad_sigs[gb] = bytes(oc)
    bad_ids[gs] = id_sets[gs][:32 * 3] + b32(0) + id_sets[gs][32 * 4:]
    out2, st2 = eng.threshold_combine_batch(bad_ids, bad_sigs)
    assert list(st2) == [ERR_G1 if g == gb else ERR_SCALAR if g == gs else 0 for g in range(len(sizes))]
    for g in range(len(sizes)):
        assert out2[64 * g:64 * g + 64] == (IDENT1 if g in (gb, gs) else out[64 * g:64 * g + 64]), g
    # ... and a bad id in the group that is handed over
    bad_ids[gb] = id_sets[gb][:-32] + id_sets[gb][:32]
    out3, st3 = eng.threshold_combine_batch(bad_ids, sig_sets)
    assert st3[gb] == ERR_SCALAR and out3[64 * gb:64 * gb + 64] == IDENT1
    lam3, lst3 = eng.lagrange_at_zero_batch(bad_ids)
    assert lst3[gb] == ERR_SCALAR and lst3[gs] == ERR_SCALAR and sum(lst3) == 2 * ERR_SCALAR
    pos = sum(sizes[:gb])
    assert lam3[32 * pos:32 * (pos + T + 1)] == bytes(32 * (T + 1)) and lam3[:32 * sizes[0]] == lam[:32 * sizes[0]]


# ---------------------------------------------------------------- 7. argument errors
def test_argument_errors(eng, oracle):
    lib, ctx = eng._lib, eng._ctx
    u8 = ctypes.POINTER(ctypes.c_uint8); u64 = ctypes.POINTER(ctypes.c_uint64)
    id_sets, sig_sets = random_groups(eng, oracle, random.Random(8), [2, 2])
    ids = np.frombuffer(b"".join(id_sets), dtype=np.uint8); sigs = np.frombuffer(b"".join(sig_sets), dtype=np.uint8)
    out = np.zeros(64 * 4, dtype=np.uint8); st = np.zeros(4, dtype=np.uint8)
    pi, ps, po, pst = ids.ctypes.data_as(u8), sigs.ctypes.data_as(u8), out.ctypes.data_as(u8), st.ctypes.data_as(u8)

    def combine(off, n, c=ctx, a=pi, s=ps, o=po, t=pst):
        arr = np.ascontiguousarray(np.asarray(off, dtype=np.uint64))
        return lib.blsbn254_threshold_combine_batch(c, a, s, arr.ctypes.data_as(u64) if len(off) else None, ctypes.c_size_t(n), o, t)

    def lagrange(off, n, c=ctx, a=pi, o=po, t=pst):
        arr = np.ascontiguousarray(np.asarray(off, dtype=np.uint64))
        return lib.blsbn254_lagrange_at_zero_batch(c, a, arr.ctypes.data_as(u64) if len(off) else None, ctypes.c_size_t(n), o, t)

    for fn in (combine, lagrange):
        assert fn([0, 3, 1], 2) == E_ARG                             # decreasing offsets
        assert fn([0, (1 << 23) + 1], 1) == E_ARG                    # more than 2^23 shares
        assert fn([0, 2], 1, c=None) == E_ARG
        assert fn([0, 2], 1, a=None) == E_ARG
        assert fn([0, 2], 1, o=None) == E_ARG
        assert fn([0, 2], 1, t=None) == E_ARG
        assert fn([], 1) == E_ARG                                    # no offsets
        assert fn([0], 0) == 0 and fn([], 0, a=None, o=None, t=None) == 0
        assert fn([0, 2, 4], 2) == 0
    assert combine([0, 2], 1, s=None) == E_ARG
    assert lib.blsbn254_threshold_batch_stats(ctx, None) == E_ARG
    with pytest.raises(ValueError):
        eng.threshold_combine_batch([bytes(32)], [bytes(64), bytes(64)])
    with pytest.raises(ValueError):
        eng.threshold_combine_batch([bytes(64)], [bytes(64)])


# ---------------------------------------------------------------- 8. on a long-lived context
def test_on_a_long_lived_context(M, eng, oracle):
    import torch
    rnd = random.Random(9)
    dst = M.DEFAULT_DST
    n = 1000
    vb = synth.make_batch_gpu(eng, oracle, n, dst, pool=40, invalid_every=7, spot=4)
    sizes_a = [7] * 300 + [0, 1, 33, 100]
    sizes_b = [3, 64, 2, 65, 9] * 20
    A = random_groups(eng, oracle, rnd, sizes_a)
    B = random_groups(eng, oracle, rnd, sizes_b)
    T300 = random_groups(eng, oracle, rnd, [300])
    T7 = random_groups(eng, oracle, rnd, [7])
    ks = b"".join(b32(rnd.randrange(R)) for _ in range(500))
    P = eng.g1_mul_batch(oracle.g1_generator() * 500, b"".join(b32(rnd.randrange(1, R)) for _ in range(500)), 500)

    def pending_verify(e):
        t = synth.dev_batch(M, torch, vb[0], vb[1], vb[2])
        torch.cuda.synchronize()
        e.verify_batch_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), n, t[4].data_ptr(), dst)
        return t

    steps = [
        lambda e: e.threshold_combine_batch(*A),
        lambda e: e.threshold_combine(T300[0][0], T300[1][0], 300),
        lambda e: e.threshold_combine_batch(*B),
        lambda e: e.g1_msm(P, ks, 500),
        lambda e: e.lagrange_at_zero_batch(B[0]),
        lambda e: e.threshold_combine(T7[0][0], T7[1][0], 7),
    ]
    fresh = []
    for f in steps:
        e = M.Engine(0)
        try:
            fresh.append(f(e))
        finally:
            e.close()
    assert fresh[0][1] == bytes(len(sizes_a)) and fresh[2][1] == bytes(len(sizes_b))
    for g in (0, 301, 302, 303):
        assert fresh[0][0][64 * g:64 * g + 64] == oracle.threshold_combine(A[0][g], A[1][g], sizes_a[g]), g
    assert fresh[1] == oracle.threshold_combine(T300[0][0], T300[1][0], 300)
    e = M.Engine(0)
    try:
        e.verify_batch(vb[0], vb[1], vb[2], dst); e.verify_batch(vb[0], vb[1], vb[2], dst)      # so that the next one is enqueued on a guess
        t0 = pending_verify(e); e.synchronize()
        t = pending_verify(e)                                                                    # left pending
        got = [f(e) for f in steps]
        e.synchronize()
        assert bytes(t[4].cpu().numpy()) == synth.bitmap_of(vb[3])
    finally:
        e.close()
    for i, (a, b) in enumerate(zip(got, fresh)):
        assert a == b, "step %d differs from the same call on a context of its own" % i
