"""GPU tests (MI355X) of the distinct-message rule checked on the device: blsbn254_hash_distinct_batch and the _distinct forms of
the aggregate verify over ragged groups.  The reference of every expectation is existing code, never the new calls: dup[g] = the
64-byte outputs of hash_to_g1_batch (under the try-and-increment maps: of the CPU model of tests/g1_map_support.py) for group g's
messages are not pairwise different, by a Python set; valid = the parent's aggregate_verify_batch bit AND NOT that."""
import ctypes

import numpy as np
import pytest

from tests import expander_support as X
from tests import g1_map_support as G
from tests import msg_distinct_support as D
from tests import synth
from tests.gpu_support import eng, fresh_engine, M
from tests.helpers import bits_of

pytestmark = pytest.mark.gpu
P = synth.P
SEED = bytes(range(7, 39))


def points_of(e, msgs, dst):
    h = e.hash_to_g1_batch(msgs, dst)
    return [h[64 * i:64 * i + 64] for i in range(len(msgs))]


def flat_args(S, lead=0):
    """the flat arguments of a Signed whose first `lead` groups are pairs in front of grp_off[0]"""
    off = S.goff()
    return b"".join(S.keys), S.flat(), off[lead:], b"".join(S.sigs[lead:]), S.dst


def check_all_forms(e, S, want_dup, lead=0, seed=SEED, want_valid=None):
    """the three calls against the reference: dup = want_dup, valid = the parent's bit and not dup; returns (parent bits, valid)"""
    pks, msgs, goff, sigs, dst = flat_args(S, lead)
    n_g = len(goff) - 1
    parent = bits_of(e.aggregate_verify_batch_flat(pks, msgs, goff, sigs, dst), n_g)
    assert bits_of(e.aggregate_verify_batch_rlc_flat(pks, msgs, goff, sigs, dst, seed), n_g) == parent
    want = D.and_not(parent, want_dup)
    if want_valid is not None:
        assert want == want_valid
    assert bits_of(e.hash_distinct_batch(msgs, goff, dst), n_g) == want_dup
    v, d = e.aggregate_verify_batch_distinct_flat(pks, msgs, goff, sigs, dst)
    assert (bits_of(v, n_g), bits_of(d, n_g)) == (want, want_dup)
    v, d = e.aggregate_verify_batch_rlc_distinct_flat(pks, msgs, goff, sigs, dst, seed)
    assert (bits_of(v, n_g), bits_of(d, n_g)) == (want, want_dup)
    return parent, want


def msg(i):
    return synth.msg_of((77 << 20) + i)


# ---------------------------------------------------------------- 1. group shapes and where the repeats sit
def shapes_case():
    """three pairs in front of grp_off[0], then groups of 1, 0, 2, 3, 64, 65, 130, 4, 2 and 2 pairs"""
    it = iter(range(10 ** 6))
    fresh = lambda k: [msg(next(it)) for _ in range(k)]
    lead = fresh(3)
    g1 = [lead[1]]                                         # equals a message in front of grp_off[0]: that pair is in no group
    g2 = fresh(1) * 2                                      # adjacent
    g3 = fresh(2); g3.append(g3[0])                        # first against last
    g64 = fresh(64)
    g65 = fresh(64); g65.append(g65[0])                    # pairs 0 and 64: two waves of one group
    g65[7] = g64[7]                                        # the same message in two different groups: not a repeat
    g130 = fresh(1) * 130                                  # all equal
    g4 = fresh(2); g4 = [g4[0], g4[1], g4[0], g4[0]]       # a triple
    sets = [lead, g1, [], g2, g3, g64, g65, g130, g4, [b"", b""], [b"", b"\x00"]]
    want = [False, False, True, True, False, True, True, True, True, False]
    return sets, want


def test_group_shapes_and_repeat_positions(eng, M):
    sets, want_dup = shapes_case()
    S = D.Signed(eng, sets, M.DEFAULT_DST)
    pts = points_of(eng, S.flat(), S.dst)
    assert D.dup_of(pts, S.goff()[1:]) == want_dup         # the reference says what the case was built to be
    parent, valid = check_all_forms(eng, S, want_dup, lead=1)
    assert parent == [True, False] + [True] * 8            # honestly signed: a repeated message does not fail the equation
    assert valid == [True, False, False, False, True, False, False, False, False, True]


# ---------------------------------------------------------------- 2. a group cut across two Miller launches
def test_repeat_across_a_launch_boundary(M, monkeypatch):
    e = fresh_engine(M, monkeypatch, "8")                  # launches of 8 lanes = 16 slots
    try:
        a, b, c = [msg(1000 + i) for i in range(5)], [msg(2000 + i) for i in range(40)], [msg(3000 + i) for i in range(37)]
        b[39] = b[0]                                       # the two equal messages lie in different launches
        S = D.Signed(e, [a, b, c, [msg(1), msg(2), msg(1)]], M.DEFAULT_DST)
        want_dup = [False, True, False, True]
        assert D.dup_of(points_of(e, S.flat(), S.dst), S.goff()) == want_dup
        before = e.aggregate_batch_stats()["launches"]
        check_all_forms(e, S, want_dup, want_valid=[True, False, True, False])
        assert e.aggregate_batch_stats()["launches"] - before >= 2 * 5       # the exact pipeline ran in several launches per call
    finally:
        e.close()


# ---------------------------------------------------------------- 3. why the call exists: the rogue-key group
def g2_neg(pk):
    neg = lambda b: ((P - int.from_bytes(b, "big")) % P).to_bytes(32, "big")
    return pk[:64] + neg(pk[64:96]) + neg(pk[96:128])


def test_rogue_key_group(eng, M):
    dst = M.DEFAULT_DST
    one = (1).to_bytes(32, "big")
    g2gen = eng.sk_to_pk_batch(one, 1)
    pk1 = eng.sk_to_pk_batch(synth.sk_of(5).to_bytes(32, "big"), 1)          # an honest key; its secret is not used below
    a = (0x1234567890abcdef << 64 | 0xfedcba) .to_bytes(32, "big")
    pk2 = eng.aggregate_pks(eng.g2_mul_batch(g2gen, a, 1) + g2_neg(pk1), 2)   # [a] G2gen - pk1
    m = b"pay the attacker"
    forged = eng.sign_batch(a, [m], dst)                                      # [a] H(m): nobody holding pk1's secret signed
    honest = D.Signed(eng, [[msg(50), msg(51)]], dst)
    keys, msgs, goff = pk1 + pk2 + honest.keys[0], [m, m] + honest.msgs[0], [0, 2, 4]
    sigs = forged + honest.sigs[0]
    assert bits_of(eng.aggregate_verify_batch_flat(keys, msgs, goff, sigs, dst), 2) == [True, True]      # the forgery passes the equation
    assert D.dup_of(points_of(eng, msgs, dst), goff) == [True, False]
    for call in (lambda: eng.aggregate_verify_batch_distinct_flat(keys, msgs, goff, sigs, dst),
                 lambda: eng.aggregate_verify_batch_rlc_distinct_flat(keys, msgs, goff, sigs, dst, SEED)):
        v, d = call()
        assert (bits_of(v, 2), bits_of(d, 2)) == ([False, True], [True, False])


# ---------------------------------------------------------------- 4. points, not bytes: the try-and-increment maps
def adjacent_winners():
    """two digests x0, x0 + 1 whose searches both stop at once: neighbours, different points"""
    x = G.WINDOW + (1 << 40)
    while not (G.is_residue(x) and G.is_residue(x + 1)):
        x += 1
    return x.to_bytes(32, "big"), (x + 1).to_bytes(32, "big")


def test_tai_digest_repeats_that_bytes_do_not_show(M, monkeypatch):
    e = fresh_engine(M, monkeypatch, None)
    try:
        e.set_g1_map(M.G1MAP_TAI_DIGEST)
        h = G.digests_with_run(0, 1)[0]
        twin = (int.from_bytes(h, "big") + P).to_bytes(32, "big")           # h < 2^256 - p: a different message, the same x0
        skipped = G.digests_with_run(1, 1)[0]                                 # its x0 fails the square test ...
        nxt = (int.from_bytes(skipped, "big") + 1).to_bytes(32, "big")        # ... so its point is that of x0 + 1
        w0, w1 = adjacent_winners()
        clean = G.digests_with_run(2, 3, skip=1)
        sets = [[h, clean[0], twin], [skipped, nxt], [w0, w1], [clean[1], h], [clean[2], nxt, clean[0]]]
        for ms in sets:
            assert len(set(ms)) == len(ms)                                    # as BYTES every group is distinct
        S = D.Signed(e, sets, M.DEFAULT_DST)
        model = [G.hash_bytes(G.TAI_DIGEST, 0, m) for m in S.flat()]
        assert points_of(e, S.flat(), S.dst) == model
        want_dup = D.dup_of(model, S.goff())
        assert want_dup == [True, True, False, False, False]
        S.corrupt(3)
        check_all_forms(e, S, want_dup, want_valid=[False, False, True, False, True])
    finally:
        e.close()


def test_tai_hash_under_keccak(M, monkeypatch):
    e = fresh_engine(M, monkeypatch, None)
    try:
        e.set_expander(M.EXPAND_XMD_KECCAK256)
        e.set_g1_map(M.G1MAP_TAI_HASH)
        sets = [[msg(1), msg(2), msg(3)], [msg(4), b"", msg(5), b""], [msg(1)], [msg(6), msg(7)] * 33]
        S = D.Signed(e, sets, M.DEFAULT_DST)
        model = [G.hash_bytes(G.TAI_HASH, X.XMD_KECCAK256, m) for m in S.flat()]
        want_dup = D.dup_of(model, S.goff())
        assert want_dup == [False, True, False, True]
        check_all_forms(e, S, want_dup, want_valid=[True, False, True, False])
    finally:
        e.close()


# ---------------------------------------------------------------- 5. both verify forms, corrupted groups among repeated ones
def mixed_case(e, dst, pool):
    sets = [[msg(100 * g + j) for j in range(k)] for g, k in enumerate([3, 5, 2, 7, 1, 4, 6, 2, 3, 5])]
    for g, (i, j) in {1: (0, 4), 3: (2, 3), 6: (5, 0), 8: (1, 2)}.items():
        sets[g][i] = sets[g][j]
    S = D.Signed(e, sets, dst, pool=pool)
    for g in (0, 3, 7):                                    # a corrupted clean group, a corrupted repeated one, another clean one
        S.corrupt(g)
    want_dup = [g in (1, 3, 6, 8) for g in range(10)]
    assert D.dup_of(points_of(e, S.flat(), dst), S.goff()) == want_dup
    return S, want_dup, [g not in (0, 1, 3, 6, 7, 8) for g in range(10)]


def test_rlc_form_on_a_repeating_key_pool(eng, M):
    S, want_dup, want_valid = mixed_case(eng, M.DEFAULT_DST, 4)
    before = eng.aggregate_rlc_stats()
    check_all_forms(eng, S, want_dup, want_valid=want_valid)
    after = eng.aggregate_rlc_stats()
    assert after["calls"] - before["calls"] == 2 and after["exact_calls"] == before["exact_calls"]
    assert after["equations"] - before["equations"] >= 2                      # the combination ran, in the parent and in the new form


def test_rlc_form_on_distinct_keys_takes_the_exact_route(eng, M):
    S, want_dup, want_valid = mixed_case(eng, M.DEFAULT_DST, 38)              # as many keys as pairs
    before = eng.aggregate_rlc_stats()
    check_all_forms(eng, S, want_dup, want_valid=want_valid)
    after = eng.aggregate_rlc_stats()
    assert after["exact_calls"] - before["exact_calls"] == 2 and after["equations"] == before["equations"]


def test_null_dup_bitmap_and_argument_errors(eng, M):
    S, want_dup, want_valid = mixed_case(eng, M.DEFAULT_DST, 4)
    pks, msgs, goff, sigs, dst = flat_args(S)
    data, off = M.engine.pack_messages(msgs)
    go = np.asarray(goff, dtype=np.uint64)
    lib, ctx = eng._lib, eng._ctx
    buf = lambda b: ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p)
    for name, extra in (("blsbn254_aggregate_verify_batch_distinct", ()), ("blsbn254_aggregate_verify_batch_rlc_distinct", (buf(SEED),))):
        valid = np.full(2, 0xff, dtype=np.uint8)
        rc = getattr(lib, name)(ctx, buf(pks), buf(data), off.ctypes, go.ctypes, buf(sigs), 10, buf(dst), len(dst), *extra, valid.ctypes, None)
        assert rc == 0 and bits_of(valid.tobytes(), 10) == want_valid
        assert getattr(lib, name)(ctx, buf(pks), buf(data), off.ctypes, go.ctypes, buf(sigs), 10, buf(dst), len(dst), *extra, None, None) == -1
    dup = np.zeros(2, dtype=np.uint8)
    assert lib.blsbn254_hash_distinct_batch(ctx, buf(data), off.ctypes, go.ctypes, 10, buf(dst), len(dst), None) == -1
    assert lib.blsbn254_hash_distinct_batch(ctx, buf(data), off.ctypes, None, 10, buf(dst), len(dst), dup.ctypes) == -1
    assert lib.blsbn254_hash_distinct_batch(ctx, buf(data), off.ctypes, go.ctypes, 0, buf(dst), len(dst), None) == 0      # no groups: nothing written
    bad = go.copy(); bad[3] = bad[2] - 1
    assert lib.blsbn254_hash_distinct_batch(ctx, buf(data), off.ctypes, bad.ctypes, 10, buf(dst), len(dst), dup.ctypes) == -1
    assert lib.blsbn254_msg_distinct_stats(ctx, None) == -1
    # every group empty: none is repeated, all are invalid
    assert bits_of(eng.hash_distinct_batch(msgs, [5, 5, 5, 5], dst), 3) == [False] * 3
    v, d = eng.aggregate_verify_batch_distinct_flat(pks, msgs, [5, 5, 5, 5], sigs[:192], dst)
    assert (bits_of(v, 3), bits_of(d, 3)) == ([False] * 3, [False] * 3)
    v, d = eng.aggregate_verify_batch_rlc_distinct_flat(pks, msgs, [5, 5, 5, 5], sigs[:192], dst, SEED)
    assert (bits_of(v, 3), bits_of(d, 3)) == ([False] * 3, [False] * 3)


# ---------------------------------------------------------------- 6. one context, several calls
def test_call_sequence_on_one_context(M, monkeypatch):
    """130 -> 3 -> 130 pairs, repeated and clean inputs alternating: stale table contents would show as wrong dup bits"""
    dst = M.DEFAULT_DST
    big_rep = [[msg(i) for i in range(64)], [msg(64 + i) for i in range(66)]]
    big_rep[1][65] = big_rep[1][0]
    small_clean = [[msg(0), msg(64)], [msg(1)]]            # messages the table of the call before held, now in other groups
    big_clean = [[msg(64 + i) for i in range(66)], [msg(i) for i in range(64)]]
    small_rep = [[msg(64), msg(64)], [msg(1)]]
    seq = [big_rep, small_clean, big_clean, small_rep, big_rep]
    want = [[False, True], [False, False], [False, False], [True, False], [False, True]]
    e = fresh_engine(M, monkeypatch, None)
    try:
        cases = [D.Signed(e, sets, dst) for sets in seq]
        stats, inserted, repeated = e.msg_distinct_stats(), 0, 0
        assert stats == dict(zip(D.MD_STATS, (0, 0, 0, 0)))
        for k, (S, want_dup) in enumerate(zip(cases, want)):
            assert D.dup_of(points_of(e, S.flat(), dst), S.goff()) == want_dup
            pks, msgs, goff, sigs, _ = flat_args(S)
            form = (e.aggregate_verify_batch_distinct_flat, lambda *a: e.aggregate_verify_batch_rlc_distinct_flat(*a, SEED),
                    lambda p, m, g, s, d: (None, e.hash_distinct_batch(m, g, d)))[k % 3]
            agb = e.aggregate_batch_stats()
            got = form(pks, msgs, goff, sigs, dst)
            agb = {n: v - agb[n] for n, v in e.aggregate_batch_stats().items()}
            f = fresh_engine(M, monkeypatch, None)
            try:
                fform = (f.aggregate_verify_batch_distinct_flat, lambda *a: f.aggregate_verify_batch_rlc_distinct_flat(*a, SEED),
                         lambda p, m, g, s, d: (None, f.hash_distinct_batch(m, g, d)))[k % 3]
                assert got == fform(pks, msgs, goff, sigs, dst), k
                # the inner pipeline is the parent's: the same counts as the parent call leaves on a fresh context
                parent = (f.aggregate_verify_batch_flat, lambda *a: f.aggregate_verify_batch_rlc_flat(*a, SEED), lambda *a: None)[k % 3]
                pb = f.aggregate_batch_stats()
                pv = parent(pks, msgs, goff, sigs, dst)
                assert agb == {n: v - pb[n] for n, v in f.aggregate_batch_stats().items()}, k
            finally:
                f.close()
            assert bits_of(got[1], 2) == want_dup, k
            if got[0] is not None:
                assert bits_of(got[0], 2) == D.and_not(bits_of(pv, 2), want_dup) == D.and_not([True, True], want_dup), k
            inserted += len(msgs); repeated += sum(want_dup)
            assert e.msg_distinct_stats() == {"calls": k + 1, "pairs": inserted, "repeated_groups": repeated, "slots": D.slots_for(len(msgs))}, k
    finally:
        e.close()
