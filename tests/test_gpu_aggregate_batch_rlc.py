"""GPU tests (MI355X) of the aggregate verify over ragged groups by random linear combination across groups
(blsbn254_aggregate_verify_batch_rlc): every bitmap is compared with blsbn254_aggregate_verify_batch on the same arguments and
with the pattern known by construction, and every case asserts what the counters of the call say, so that equality is never
reached merely through the exact sub-call.  Data is signed by the engine's own sign_batch over a pool of 8 keys."""
import ctypes

import numpy as np
import pytest

from tests import point_cases, synth
from tests.aggregate_rlc_support import AGR_STATS, Data, SEED, cut
from tests.gpu_support import MILLER_KERNELS, eng, fresh_engine, launches, M
from tests.helpers import bits_of, IDENT1, IDENT2, offsets_u64

pytestmark = pytest.mark.gpu
R = synth.R
E_ARG = -1
SEED_B = bytes(range(101, 133))


def run(e, D, seed=SEED):
    """(bits of the RLC call, what its counters and the exact call's group counter moved by); the bitmap equals the exact call's"""
    s0, a0 = e.aggregate_rlc_stats(), e.aggregate_batch_stats()["groups"]
    got = e.aggregate_verify_batch_rlc(*D.args(), seed)
    s1, a1 = e.aggregate_rlc_stats(), e.aggregate_batch_stats()["groups"]
    delta = {k: s1[k] - s0[k] for k in AGR_STATS}
    delta["pipeline_groups"] = a1 - a0
    assert got == e.aggregate_verify_batch(*D.args())
    return bits_of(got, len(D.sizes)), delta


def stats(calls=1, round1=0, round2=0, exact=0, ineligible=0, equations=1, exact_calls=0, failed=0, pipeline=0):
    return dict(zip(AGR_STATS + ("pipeline_groups",), (calls, round1, round2, exact, ineligible, equations, exact_calls, failed, pipeline)))


@pytest.fixture
def segments(eng):
    """eng.set_aggregate_rlc_segments for one test, the default rule restored afterwards"""
    yield eng.set_aggregate_rlc_segments
    eng.set_aggregate_rlc_segments(0)


# ---------------------------------------------------------------- 1. ragged honest batch
def test_ragged_honest_batch(eng, M):
    sizes = [1, 2, 3, 4, 5, 7, 1, 8] * 5
    D = Data(eng, sizes, M.DEFAULT_DST, salt=1)
    bits, delta = run(eng, D)
    assert bits == [True] * 40
    assert delta == stats(round1=40)
    s0 = eng.aggregate_batch_stats()
    got, rec = launches(eng, lambda: eng.aggregate_verify_batch_rlc(*D.args(), SEED), MILLER_KERNELS)
    assert bits_of(got, 40) == [True] * 40
    assert "miller_hpk2r" not in rec and sum(rec.values()) == 1, rec
    assert eng.aggregate_batch_stats() == s0


# ---------------------------------------------------------------- 2. damage classes
DAMAGE = ("wrong_message", "undecodable_sig", "off_curve_sig", "identity_sig", "off_curve_key", "outside_key", "identity_key", "empty_group")


@pytest.mark.parametrize("kind", DAMAGE)
def test_one_damaged_group_among_honest_ones(eng, M, oracle, pyref, segments, kind):
    n_g, bad = 12, 7
    D = Data(eng, [3] * n_g, M.DEFAULT_DST, salt=2)
    s = D.sigs[bad]
    if kind == "wrong_message":
        D.flip_message(bad, 1)
    elif kind == "undecodable_sig":
        D.sigs[bad] = b"\xff" * 32 + s[32:]
    elif kind == "off_curve_sig":
        D.sigs[bad] = s[:63] + bytes([s[63] ^ 1])
    elif kind == "identity_sig":
        D.sigs[bad] = IDENT1
    elif kind == "off_curve_key":
        k = D.keys[bad][2]
        D.keys[bad][2] = k[:127] + bytes([k[127] ^ 1])
    elif kind == "outside_key":
        D.keys[bad][1] = point_cases.g2_cases(oracle, pyref)["outside_0"][1]
    elif kind == "identity_key":
        D.keys[bad][0] = IDENT2
    else:
        D.keys[bad], D.msgs[bad] = [], []
    want = [g != bad for g in range(n_g)]
    if kind != "wrong_message":
        bits, delta = run(eng, D)
        assert bits == want
        assert delta == stats(round1=n_g - 1, ineligible=1)          # not eligible: no equation, no exact sub-call spent on it
        return
    segments(4)
    bound, seg_of = cut(n_g, 4)
    mine = bound[seg_of[bad] + 1] - bound[seg_of[bad]]                  # every group is eligible: the failed segment's groups
    bits, delta = run(eng, D)
    assert bits == want
    assert delta == stats(round2=n_g - mine, exact=mine, equations=5, failed=1, pipeline=mine)


# ---------------------------------------------------------------- 3. errors that cancel without weights
@pytest.mark.parametrize("seed", [SEED, SEED_B], ids=["seed_a", "seed_b"])
@pytest.mark.parametrize("kind", ["plus_minus_d", "sigs_swapped", "messages_swapped"])
def test_errors_that_cancel_without_weights(eng, M, oracle, kind, seed):
    n_g, a, b = 8, 0, 2                                                 # both in the first of the default rule's 2 segments (32 pairs, 8 keys)
    D = Data(eng, [4] * n_g, M.DEFAULT_DST, salt=3)
    if kind == "plus_minus_d":
        d = oracle.g1_mul(oracle.g1_generator(), 777)
        D.sigs[a], D.sigs[b] = oracle.g1_add(D.sigs[a], d), oracle.g1_add(D.sigs[b], oracle.g1_mul(d, R - 1))
    elif kind == "sigs_swapped":
        D.sigs[a], D.sigs[b] = D.sigs[b], D.sigs[a]
    else:
        assert D.keys[a][0] == D.keys[b][0]                             # pair 0 of both groups is under key 0
        D.msgs[a][0], D.msgs[b][0] = D.msgs[b][0], D.msgs[a][0]
    bits, delta = run(eng, D, seed)
    assert bits == [g not in (a, b) for g in range(n_g)]
    assert delta == stats(round2=4, exact=4, equations=3, failed=1, pipeline=4)


# ---------------------------------------------------------------- 4. repeated keys and messages inside a group
def test_repeated_keys_and_messages(eng, M):
    D = Data(eng, [3, 2, 2, 2, 3], M.DEFAULT_DST, pool=3, salt=4)
    skb = [synth.sk_of(k).to_bytes(32, "big") for k in range(3)]
    pk = [D.keys[0][0], D.keys[0][1], D.keys[0][2]]
    m = synth.msg_of(77)

    def group(g, ks, ms):
        D.keys[g], D.msgs[g] = [pk[k] for k in ks], ms
        sigs = eng.sign_batch(b"".join(skb[k] for k in ks), ms, D.dst)
        D.sigs[g] = eng.aggregate_sigs(sigs, len(ks))

    group(0, [0, 0, 1], D.msgs[0])                                      # one key twice in a group (and in groups 1 and 3)
    group(2, [1, 2], [m, m])                                            # one message twice in a group, under two keys
    group(3, [0, 0], [m, m])                                            # the same pair twice
    bits, delta = run(eng, D)
    assert bits == [True] * 5 and delta == stats(round1=5)
    D.flip_message(3, 1)
    bits, delta = run(eng, D)
    assert bits == [True, True, True, False, True]
    assert delta["round1_groups"] == 0 and delta["exact_groups"] + delta["round2_groups"] == 5 and delta["exact_groups"] >= 1


# ---------------------------------------------------------------- 5. all-distinct keys
def test_distinct_keys_take_the_exact_call(eng, M):
    D = Data(eng, [1] * 16, M.DEFAULT_DST, pool=16, salt=5)             # u = 16 keys among 16 pairs: 2 u > N
    D.flip_message(9)
    bits, delta = run(eng, D)
    assert bits == [g != 9 for g in range(16)]
    assert delta == stats(exact=16, equations=0, exact_calls=1, pipeline=16)


# ---------------------------------------------------------------- 6. offsets that do not start at 0, empty groups at both ends
def test_group_offsets_need_not_start_at_zero(eng, M, segments):
    dst = M.DEFAULT_DST
    D = Data(eng, [2, 0, 3, 2, 4, 3, 4, 0], dst, salt=6)
    keys, msgs = b"".join(b"".join(k) for k in D.keys), [m for ms in D.msgs for m in ms]
    goff = offsets_u64(D.sizes)[1:]                                       # the first group's two pairs belong to no group
    sigs = b"".join(D.sigs[1:])

    def both(msgs):
        s0 = eng.aggregate_rlc_stats()
        got = eng.aggregate_verify_batch_rlc_flat(keys, msgs, goff, sigs, dst, SEED)
        s1 = eng.aggregate_rlc_stats()
        assert got == eng.aggregate_verify_batch_flat(keys, msgs, goff, sigs, dst)
        return bits_of(got, 7), {k: s1[k] - s0[k] for k in AGR_STATS}

    bits, delta = both(msgs)
    assert bits == [False, True, True, True, True, True, False]
    assert delta == {k: v for k, v in stats(round1=5, ineligible=2).items() if k != "pipeline_groups"}
    # damage in the leading pairs changes nothing; a wrong message in the last non-empty group: its segment alone goes to the exact
    # pipeline, trimmed to its eligible groups (7 groups in 3 segments: 0 1 | 2 3 | 4 5 6)
    msgs2 = [b"other", b""] + msgs[2:]
    msgs2[2 + 3 + 2 + 4 + 3] = b"wrong"
    segments(3)
    a0 = eng.aggregate_batch_stats()["groups"]
    bits, delta = both(msgs2)
    assert bits == [False, True, True, True, True, False, False]
    assert delta == {k: v for k, v in stats(round2=3, exact=2, ineligible=2, equations=4, failed=1).items() if k != "pipeline_groups"}
    assert eng.aggregate_batch_stats()["groups"] - a0 == 2 + 7            # the trimmed range, and the exact call of both()


# ---------------------------------------------------------------- 7. segment forms over several launches
def test_segments_span_several_launches(M, monkeypatch):
    """... in the form that fits each launch: a wave per slot, and one slot per lane on an engine without the wave and quad
    kernels -- never two slots per lane in a second round, where a lane's value must belong to one segment"""
    for knobs, kernel in (({}, "miller_wide_1p"), ({"BLSBN254_WIDE_FE": "0", "BLSBN254_TRI_MAX": "0"}, "miller_hpk1p")):
        e = fresh_engine(M, monkeypatch, "64", knobs)                    # 4 x (33 + 1) Miller slots: three launches of at most 64
        try:
            n_g = 24
            D = Data(e, [3] * n_g, M.DEFAULT_DST, pool=33, salt=7)
            e.set_aggregate_rlc_segments(4)
            bits, delta = run(e, D)
            assert bits == [True] * n_g and delta == stats(round1=n_g)
            D.flip_message(n_g - 2, 2)                                   # in the last of the 4 segments of 6 groups
            want = [g != n_g - 2 for g in range(n_g)]
            (bits, delta), rec = launches(e, lambda: run(e, D), MILLER_KERNELS)
            assert bits == want and delta == stats(round2=18, exact=6, equations=5, failed=1, pipeline=6)
            assert rec.get(kernel, 0) == 1 + 3, rec                       # round 1: 34 slots; round 2: 136 slots, 64 + 64 + 8
            assert set(rec) == {kernel, "miller_hpk2r"}, rec              # (the exact pipeline's own loop: the failed segment, and run()'s exact call)
            e.set_aggregate_rlc_segments(1)                              # no second round: every eligible group to the exact pipeline
            bits, delta = run(e, D)
            assert bits == want and delta == stats(exact=n_g, pipeline=n_g)
        finally:
            e.close()


# ---------------------------------------------------------------- 8. seed = None, argument errors
def test_seed_from_the_os_and_argument_errors(eng, M, segments):
    lib, ctx = eng._lib, eng._ctx
    u8 = ctypes.POINTER(ctypes.c_uint8); u64 = ctypes.POINTER(ctypes.c_uint64)
    dst = M.DEFAULT_DST
    D = Data(eng, [3] * 8, dst, salt=8)
    D.flip_message(5)
    bits, delta = run(eng, D, None)
    assert bits == [g != 5 for g in range(8)] and delta["round1_groups"] == 0 and delta["exact_groups"] >= 1
    G = Data(eng, [2, 2], dst, pool=2, salt=9)
    pk = np.frombuffer(b"".join(b"".join(k) for k in G.keys), dtype=np.uint8); ms = np.frombuffer(b"".join(m for x in G.msgs for m in x), dtype=np.uint8)
    sg = np.frombuffer(b"".join(G.sigs), dtype=np.uint8); d = np.frombuffer(dst, dtype=np.uint8); sd = np.frombuffer(SEED, dtype=np.uint8)
    off = np.arange(0, 32 * 5, 32, dtype=np.uint64)
    out = np.zeros(8, dtype=np.uint8)
    P = lambda a: a.ctypes.data_as(u8)
    fn = lib.blsbn254_aggregate_verify_batch_rlc

    def call(goff, n, pks=P(pk), msgs=P(ms), o=off, sigs=P(sg), tag=P(d), bm=P(out), c=ctx, seed=P(sd)):
        arr = np.ascontiguousarray(np.asarray(goff, dtype=np.uint64))
        return fn(c, pks, msgs, o.ctypes.data_as(u64) if o is not None else None, arr.ctypes.data_as(u64) if len(goff) else None, sigs,
                  ctypes.c_size_t(n), tag, ctypes.c_size_t(len(dst)), seed, bm)

    assert call([0, 2, 4], 2) == 0 and out[0] == 3
    out[0] = 0
    assert call([0, 2, 4], 2, seed=None) == 0 and out[0] == 3
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
    assert call([0], 0) == 0 and call([], 0, pks=None, msgs=None, o=None, sigs=None, tag=None, bm=None, seed=None) == 0
    assert lib.blsbn254_aggregate_rlc_stats(ctx, None) == E_ARG
    assert lib.blsbn254_aggregate_rlc_stats(None, (ctypes.c_uint64 * 8)()) == E_ARG
    assert lib.blsbn254_set_aggregate_rlc_segments(ctx, ctypes.c_size_t(4097)) == E_ARG
    assert lib.blsbn254_set_aggregate_rlc_segments(None, ctypes.c_size_t(4)) == E_ARG
    segments(4096)
    assert eng.aggregate_verify_batch_rlc([], [], b"", dst) == b""
    s0 = eng.aggregate_rlc_stats()
    assert eng.aggregate_verify_batch_rlc([b"", b""], [[], []], b"".join(G.sigs), dst) == b"\x00"     # empty groups only: invalid
    s1 = eng.aggregate_rlc_stats()
    assert {k: s1[k] - s0[k] for k in AGR_STATS} == {k: v for k, v in stats(ineligible=2, equations=0).items() if k != "pipeline_groups"}
    with pytest.raises(ValueError):
        eng.aggregate_verify_batch_rlc([b"".join(k) for k in G.keys], [G.msgs[0]], b"".join(G.sigs), dst)
    with pytest.raises(ValueError):
        eng.aggregate_verify_batch_rlc([b"".join(k) for k in G.keys], [G.msgs[0], G.msgs[1][:1]], b"".join(G.sigs), dst)


# ---------------------------------------------------------------- 9. a sequence on one context
def test_sequence_on_one_context(eng, M, oracle):
    """verify_batch under tag 1, the RLC call under tag 2 with a failing group, the exact call under tag 1 (every group invalid
    there), the RLC call again: each result equals the same call on a context of its own"""
    tag1 = M.DEFAULT_DST
    tag2 = tag1[:-1] + bytes([tag1[-1] ^ 1])
    V = synth.make_batch(oracle, 40, tag1, pool=8, invalid_every=7, uniq=40)
    D = Data(eng, [3] * 10, tag2, salt=10)
    D.flip_message(4)
    keys, msgs, sigs, _ = D.args()
    calls = [lambda e: e.verify_batch(V[0], V[1], V[2], tag1),
             lambda e: e.aggregate_verify_batch_rlc(keys, msgs, sigs, tag2, SEED),
             lambda e: e.aggregate_verify_batch(keys, msgs, sigs, tag1),
             lambda e: e.aggregate_verify_batch_rlc(keys, msgs, sigs, tag2, SEED_B)]
    want = []
    for f in calls:
        fresh = M.Engine(0)
        try:
            want.append(f(fresh))
        finally:
            fresh.close()
    assert want[0] == synth.bitmap_of(V[3]) and want[2] == bytes(2)
    assert bits_of(want[1], 10) == bits_of(want[3], 10) == [g != 4 for g in range(10)]
    e = M.Engine(0)
    try:
        assert [f(e) for f in calls] == want
        assert e.aggregate_rlc_stats()["calls"] == 2
    finally:
        e.close()
