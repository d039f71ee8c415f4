"""GPU tests (MI355X) of the wire-format forms of the checked aggregation, the checked merge and the committee verify
(blsbn254_keyset_*_checked_batch_compressed, blsbn254_keyset_committee_fast_aggregate_verify_batch_compressed).  The contract
is stated by composition and tested that way: every expected value is the UNCOMPRESSED call on g1_inflate_batch of the same
signatures, its out_sigs through g1_compress_batch -- status, rows, used flags and the stats delta byte for byte.  The
uncompressed calls are pinned to the oracle by their own tests."""
import ctypes
import random

import numpy as np
import pytest

import blsbn254_loader
from tests import synth
from tests.gpu_support import eng, M
from tests.helpers import b32, bits_of, row_of
from tests.keyset_support import Committee, compress_entries, compressed, delta, good_keys, sign_sets, ST_SHORT

pytestmark = pytest.mark.gpu
E_ARG = -1
P = synth.P
_M = blsbn254_loader.load()
_M.Engine.keyset_aggregate_checked_batch_compressed         # the feature is there, or this module does not import
u8, u32, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
X_BIG = b32(P + 5)                                           # x >= p
IDENT_W = (bytes(32), bytes([0x80]) + bytes(31))             # the identity with either flag
NO_POINT = next(b32(x) for x in range(2, 99) if pow(x ** 3 + 3, (P - 1) // 2, P) == P - 1)     # x^3 + 3 is no square


def flip_flag(c):
    return bytes([c[0] ^ 0x80]) + c[1:]


def inflate_entries(e, wire):
    """[{slot: 32 bytes}] -> [{slot: 64 bytes, the marker where it does not inflate}]"""
    flat = [(g, k) for g, es in enumerate(wire) for k in sorted(es)]
    f = e.g1_inflate_batch(b"".join(wire[g][k] for g, k in flat), len(flat))[0] if flat else b""
    out = [dict() for _ in wire]
    for j, (g, k) in enumerate(flat):
        out[g][k] = f[64 * j:64 * j + 64]
    return out


# ------------------------------------------------------------------ the collector, key-set form
def collector_case(e, com, dst):
    """groups 0 .. 5 of sizes 20, 3, 0, 11, 1, 9 (as many as the set has good keys): 0 has one signature made with a wrong
    secret key and 1 one with the sign flag flipped (both go to the fallback); 2 is empty (short); 3 carries, on spare keys, an
    x >= p, an x with no point, the identity with either flag and an entry on a bad key (all left out, no fallback); 6 and 7
    hold one undecodable entry / one identity each (short, no fallback).  Returns (wire entries, msgs)."""
    rnd = random.Random(81)
    good = [i for i in good_keys(com) if i != com.at.get("negp")]
    sets = [set(rnd.sample(good, min(s, len(good)))) for s in (20, 3, 0, 11, 1, 9)] + [{good[0]}, {good[-1]}]
    msgs = [b"wire collector %d" % g for g in range(len(sets))]
    wrong = (0, sorted(sets[0])[min(13, len(sets[0]) - 1)])
    wire = compress_entries(e, sign_sets(e, com, sets, msgs, dst, sk=lambda g, i: com.sk[i] + 1 if (g, i) == wrong else None))
    k = sorted(sets[1])[-1]
    wire[1][k] = flip_flag(wire[1][k])
    spare = [i for i in good if i not in sets[3]]
    donor = wire[3][min(sets[3])]
    for i, junk in zip(spare, (X_BIG, NO_POINT, IDENT_W[0], IDENT_W[1], flip_flag(X_BIG))):
        wire[3][i] = junk
    if com.at:
        wire[3][com.at["off"]] = donor                                   # a good signature on a key that fails KeyValidate
    wire[6][good[0]] = X_BIG
    wire[7][good[-1]] = IDENT_W[1]
    return wire, msgs


def collector_both(e, ks, wire, msgs, dst):
    """(the compressed call, what the contract makes of the uncompressed one, the two stats deltas)"""
    s0 = e.keyset_aggregate_stats()
    got = e.keyset_aggregate_checked_batch_compressed(ks, wire, msgs, dst)
    s1 = e.keyset_aggregate_stats()
    ref = e.keyset_aggregate_checked_batch(ks, inflate_entries(e, wire), msgs, dst)
    s2 = e.keyset_aggregate_stats()
    return got, (compressed(e, ref[0]), ref[1], ref[2]), delta(s1, s0), delta(s2, s1)


@pytest.mark.parametrize("n", [1, 33, 70])
def test_collector_keyset(eng, M, n):
    dst = M.DEFAULT_DST
    com = Committee(eng, n, 300 + n)
    wire, msgs = collector_case(eng, com, dst)
    ks = M.KeySet(eng, com.pks, n)
    try:
        got, want, d_got, d_want = collector_both(eng, ks, wire, msgs, dst)
        assert eng.keyset_aggregate_checked_batch_compressed(ks, [list(w.items())[::-1] for w in wire], msgs, dst) == got       # the wrapper sorts
    finally:
        ks.close()
    assert got[2] == want[2] and got[1] == want[1] and got[0] == want[0]
    assert len(got[0]) == 32 * len(msgs)
    sizes = [min(s, n) for s in (20, 3)]
    if n == 1:                  # the only entry of groups 0 and 1 is the wrong one: the fallback leaves nothing
        assert list(got[2]) == [ST_SHORT, ST_SHORT, ST_SHORT, 0, 0, 0, ST_SHORT, ST_SHORT]
        assert d_got == d_want == {"optimistic_groups": 3, "fallback_groups": 2, "verified_signatures": 2, "short_groups": 5}
    else:
        assert list(got[2]) == [0, 0, ST_SHORT, 0, 0, 0, ST_SHORT, ST_SHORT]
        # the undecodable entries, the identities and the entry on the bad key of group 3 sent nothing to the fallback
        assert d_got == d_want == {"optimistic_groups": 3, "fallback_groups": 2, "verified_signatures": sum(sizes), "short_groups": 3}
        rb = (n + 7) // 8
        assert got[1][3 * rb:4 * rb] == row_of({i for i, c in wire[3].items() if c not in (X_BIG, NO_POINT, flip_flag(X_BIG)) + IDENT_W} - {com.at["off"]}, n)
    for g in (2, 6, 7):
        assert got[0][32 * g:32 * g + 32] == IDENT_W[1]                   # a short group: the compressed identity


# ------------------------------------------------------------------ committees: the collector, the merge, the verify
class World:
    """a registry of 140 keys (the special keys of Committee among them) and two committees of 33 and 70 members listed in
    shuffled order, each with one member that fails KeyValidate"""

    def __init__(self, eng, M):
        self.dst = M.DEFAULT_DST
        self.n = 140
        rnd = random.Random(4242)
        self.reg = reg = Committee(eng, self.n, 77)
        plain = [i for i in range(self.n) if i not in set(reg.at.values())]
        rnd.shuffle(plain)
        self.coms = [plain[:32] + [reg.at["off"]], plain[20:89] + [reg.at["undec"]]]
        for c in self.coms:
            rnd.shuffle(c)
        assert [len(c) for c in self.coms] == [33, 70] and set(self.coms[0]) & set(self.coms[1])
        self.bad_pos = [self.coms[0].index(reg.at["off"]), self.coms[1].index(reg.at["undec"])]
        self.clean = [[j for j in range(len(c)) if j != self.bad_pos[k]] for k, c in enumerate(self.coms)]

    def keyset(self, M, e):
        ks = M.KeySet(e, self.reg.pks, self.n)
        ks.set_committees(self.coms)
        return ks

    def sign(self, e, com, pos_sets, msgs, sk=None):
        """[{position: 64-byte signature of that member on msgs[g]}]; sk(g, position) overrides the signing key"""
        sets = [{self.coms[c][p] for p in ps} for c, ps in zip(com, pos_sets)]
        by_key = sign_sets(e, self.reg, sets, msgs, self.dst, sk=(lambda g, i: sk(g, self.coms[com[g]].index(i))) if sk else None)
        return [{p: by_key[g][self.coms[c][p]] for p in ps} for g, (c, ps) in enumerate(zip(com, pos_sets))]

    def aggregate(self, e, c, ps, msg, wrong=False):
        """the 64-byte aggregate of the members at positions ps of committee c on msg (wrong: of other secret keys)"""
        s = sum(self.reg.sk[self.coms[c][p]] for p in ps) % synth.R
        return e.sign_batch(b32((s + (1 if wrong else 0)) or 1), [msg], self.dst)


@pytest.fixture(scope="module")
def W(eng, M):
    return World(eng, M)


@pytest.fixture(scope="module")
def wks(eng, M, W):
    ks = W.keyset(M, eng)
    yield ks
    ks.close()


def committee_collector_case(e, W):
    """collector_case over the two committees, the groups alternating between them"""
    rnd = random.Random(82)
    com = [1, 0, 1, 0, 1, 0, 0, 1]
    pos_sets = [set(rnd.sample(W.clean[c], s)) for c, s in zip(com, (20, 3, 0, 11, 1, 9))] + [{W.clean[0][0]}, {W.clean[1][-1]}]
    msgs = [b"wire committee collector %d" % g for g in range(len(com))]
    wrong = (0, sorted(pos_sets[0])[13])
    wire = compress_entries(e, W.sign(e, com, pos_sets, msgs, sk=lambda g, p: W.reg.sk[W.coms[com[g]][p]] + 1 if (g, p) == wrong else None))
    k = sorted(pos_sets[1])[-1]
    wire[1][k] = flip_flag(wire[1][k])
    spare = [p for p in W.clean[0] if p not in pos_sets[3]]
    donor = wire[3][min(pos_sets[3])]
    for p, junk in zip(spare, (X_BIG, NO_POINT, IDENT_W[0], IDENT_W[1], flip_flag(X_BIG))):
        wire[3][p] = junk
    wire[3][W.bad_pos[0]] = donor
    wire[6][W.clean[0][0]] = NO_POINT
    wire[7][W.clean[1][-1]] = IDENT_W[0]
    return com, wire, msgs


def committee_collector_both(e, ks, W, com, wire, msgs):
    s0 = e.keyset_committee_aggregate_stats()
    got = e.keyset_committee_aggregate_checked_batch_compressed(ks, com, wire, msgs, W.dst)
    s1 = e.keyset_committee_aggregate_stats()
    ref = e.keyset_committee_aggregate_checked_batch(ks, com, inflate_entries(e, wire), msgs, W.dst)
    s2 = e.keyset_committee_aggregate_stats()
    return got, (compressed(e, ref[0]), ref[1], ref[2]), delta(s1, s0), delta(s2, s1)


def test_collector_committee(eng, W, wks):
    com, wire, msgs = committee_collector_case(eng, W)
    got, want, d_got, d_want = committee_collector_both(eng, wks, W, com, wire, msgs)
    assert got[2] == want[2] and got[1] == want[1] and got[0] == want[0]
    assert list(got[2]) == [0, 0, ST_SHORT, 0, 0, 0, ST_SHORT, ST_SHORT]
    assert d_got == d_want == {"optimistic_groups": 3, "fallback_groups": 2, "verified_signatures": 23, "short_groups": 3}
    assert [len(r) for r in got[1]] == [(len(W.coms[c]) + 7) // 8 for c in com]
    for g in (2, 6, 7):
        assert got[0][32 * g:32 * g + 32] == IDENT_W[1]


def merge_case(e, W, committee):
    """groups of 1, 3 and 16 contributions, as (positions, wire signature) lists.  0: one honest; 1: three, the second overlaps
    the first; 2: sixteen disjoint ones, the fifth wrong (the fallback drops it); 3: three, the second does not inflate (left
    out, no fallback); 4: one that does not inflate (short); 5: one wrong one (the fallback, then short).  committee: None for
    rows over the registry (positions are then read through committee 1's member list), else the committee of every group."""
    c = 1 if committee is None else committee
    clean = W.clean[c]
    span = 4 if len(clean) >= 64 else 2
    layout = [[clean[0:5]], [clean[0:4], clean[3:8], clean[8:11]], [clean[span * j:span * j + span] for j in range(16)],
              [clean[1:3], clean[5:9], clean[9:10]], [clean[2:6]], [clean[4:7]]]
    wrong = {(2, 4), (5, 0)}
    msgs = [b"wire merge %d" % g for g in range(len(layout))]
    flat = [(g, j, ps) for g, cs in enumerate(layout) for j, ps in enumerate(cs)]
    sig64 = b"".join(W.aggregate(e, c, ps, msgs[g], wrong=(g, j) in wrong) for g, j, ps in flat)
    cw = compressed(e, sig64)
    groups = [[] for _ in layout]
    for t, (g, j, ps) in enumerate(flat):
        sig = cw[32 * t:32 * t + 32]
        if (g, j) == (3, 1):
            sig = X_BIG
        if (g, j) == (4, 0):
            sig = NO_POINT
        groups[g].append(([W.coms[c][p] for p in ps] if committee is None else list(ps), sig))
    return groups, msgs


def inflate_groups(e, groups):
    flat = [sig for cs in groups for _, sig in cs]
    f = e.g1_inflate_batch(b"".join(flat), len(flat))[0]
    it = iter(f[64 * t:64 * t + 64] for t in range(len(flat)))
    return [[(row, next(it)) for row, _ in cs] for cs in groups]


MERGE_STATUS = [0, 0, 0, 0, ST_SHORT, ST_SHORT]
MERGE_USED = [[True], [True, False, True], [j != 4 for j in range(16)], [True, False, True], [False], [False]]
MERGE_DELTA = {"optimistic_groups": 3, "fallback_groups": 2, "verified_contributions": 17, "short_groups": 2}


def test_merge_keyset(eng, M, W):
    groups, msgs = merge_case(eng, W, None)
    ks = M.KeySet(eng, W.reg.pks, W.n)
    try:
        s0 = eng.keyset_merge_stats()
        got = eng.keyset_merge_checked_batch_compressed(ks, groups, msgs, W.dst)
        s1 = eng.keyset_merge_stats()
        ref = eng.keyset_merge_checked_batch(ks, inflate_groups(eng, groups), msgs, W.dst)
        s2 = eng.keyset_merge_stats()
    finally:
        ks.close()
    assert got == (compressed(eng, ref[0]), ref[1], ref[2], ref[3])
    assert list(got[3]) == MERGE_STATUS and got[2] == MERGE_USED
    assert delta(s1, s0) == delta(s2, s1) == MERGE_DELTA
    assert got[0][32 * 4:32 * 6] == IDENT_W[1] * 2


@pytest.mark.parametrize("c", [0, 1])
def test_merge_committee(eng, W, wks, c):
    groups, msgs = merge_case(eng, W, c)
    com = [c] * len(groups)
    s0 = eng.keyset_committee_merge_stats()
    got = eng.keyset_committee_merge_checked_batch_compressed(wks, com, groups, msgs, W.dst)
    s1 = eng.keyset_committee_merge_stats()
    ref = eng.keyset_committee_merge_checked_batch(wks, com, inflate_groups(eng, groups), msgs, W.dst)
    s2 = eng.keyset_committee_merge_stats()
    assert got == (compressed(eng, ref[0]), ref[1], ref[2], ref[3])
    assert list(got[3]) == MERGE_STATUS and got[2] == MERGE_USED
    assert delta(s1, s0) == delta(s2, s1) == MERGE_DELTA


def test_committee_verify(eng, W, wks):
    """the committee verify on compressed signatures: the uncompressed call's bitmap on the inflated signatures"""
    com = [0, 1, 1, 0, 1, 0]
    pos_sets = [set(W.clean[c][g:g + 5 + 3 * g]) for g, c in enumerate(com)]
    msgs = [b"wire verify %d" % g for g in range(len(com))]
    sig64 = b"".join(W.aggregate(eng, c, ps, m, wrong=(g == 2)) for g, (c, ps, m) in enumerate(zip(com, pos_sets, msgs)))
    cw = bytearray(compressed(eng, sig64))
    cw[32 * 1:32 * 2] = flip_flag(bytes(cw[32:64]))                      # -sigma
    cw[32 * 4:32 * 5] = X_BIG                                            # does not inflate
    cw[32 * 5:32 * 6] = IDENT_W[1]
    rows = [row_of(ps, len(W.coms[c])) for c, ps in zip(com, pos_sets)]
    got = eng.keyset_committee_fast_aggregate_verify_batch_compressed(wks, com, rows, msgs, bytes(cw), W.dst)
    full = eng.g1_inflate_batch(bytes(cw), len(com))[0]
    assert got == eng.keyset_committee_fast_aggregate_verify_batch(wks, com, rows, msgs, full, W.dst)
    assert [bool(b) for b in bits_of(got, len(com))] == [True, False, False, True, False, False]


# ------------------------------------------------------------------ launch boundaries, one context, the chain
def test_launch_boundaries(eng, M, W, wks, monkeypatch):
    """BLSBN254_CHUNK_LANES unset, 8 and 16 on fresh engines: the cuts fall inside a group's entries, between groups and inside
    the fallback's sub-call; the results are those of the module's engine"""
    dst = M.DEFAULT_DST
    com70 = Committee(eng, 70, 370)
    wire, msgs = collector_case(eng, com70, dst)
    ccom, cwire, cmsgs = committee_collector_case(eng, W)
    groups, mmsgs = merge_case(eng, W, None)
    cgroups, cmmsgs = merge_case(eng, W, 1)
    ks70 = M.KeySet(eng, com70.pks, 70)
    wide = M.KeySet(eng, W.reg.pks, W.n)
    try:
        want = [collector_both(eng, ks70, wire, msgs, dst)[1], committee_collector_both(eng, wks, W, ccom, cwire, cmsgs)[1]]
        ref = eng.keyset_merge_checked_batch(wide, inflate_groups(eng, groups), mmsgs, W.dst)
        want.append((compressed(eng, ref[0]),) + ref[1:])
        ref = eng.keyset_committee_merge_checked_batch(wks, [1] * len(cgroups), inflate_groups(eng, cgroups), cmmsgs, W.dst)
        want.append((compressed(eng, ref[0]),) + ref[1:])
    finally:
        ks70.close(); wide.close()
    for chunk in (None, "8", "16"):
        with monkeypatch.context() as mp:
            if chunk:
                mp.setenv("BLSBN254_CHUNK_LANES", chunk)
            e = M.Engine(0)
        try:
            k70 = M.KeySet(e, com70.pks, 70); kw = W.keyset(M, e)
            try:
                got = [e.keyset_aggregate_checked_batch_compressed(k70, wire, msgs, dst),
                       e.keyset_committee_aggregate_checked_batch_compressed(kw, ccom, cwire, cmsgs, W.dst),
                       e.keyset_merge_checked_batch_compressed(kw, groups, mmsgs, W.dst),
                       e.keyset_committee_merge_checked_batch_compressed(kw, [1] * len(cgroups), cgroups, cmmsgs, W.dst)]
                assert e.keyset_aggregate_stats() == {"optimistic_groups": 3, "fallback_groups": 2, "verified_signatures": 23, "short_groups": 3}
                assert e.keyset_merge_stats() == MERGE_DELTA and e.keyset_committee_merge_stats() == MERGE_DELTA
            finally:
                k70.close(); kw.close()
        finally:
            e.close()
        for j, (a, b) in enumerate(zip(got, want)):
            assert a == b, (chunk, j)


def test_one_context_in_sequence(eng, M):
    """the compressed collector, the uncompressed collector, verify_batch_compressed, then the compressed collector again with a
    fallback: each result equals the same call on a context of its own (the staging buffers are reused, not shared)"""
    dst = M.DEFAULT_DST
    com = Committee(eng, 70, 470)
    good = good_keys(com)
    sets = [set(good[:30]), set(good[10:12]), set(good[40:])]
    hmsgs = [b"wire sequence %d" % g for g in range(3)]
    honest64 = sign_sets(eng, com, sets, hmsgs, dst)
    honest = compress_entries(eng, honest64)
    wire, msgs = collector_case(eng, com, dst)                           # needs the fallback
    vk = good[:24]
    vmsgs = [b"wire tuple %d" % j for j in range(len(vk))]
    vs = bytearray(eng.g1_compress_batch(eng.sign_batch(b"".join(b32(com.sk[i]) for i in vk), vmsgs, dst), len(vk)))
    vs[32 * 3:32 * 4] = flip_flag(bytes(vs[96:128])); vs[32 * 9:32 * 10] = X_BIG
    vp = eng.g2_compress_batch(com.gather(vk), len(vk))
    steps = [
        lambda e, k: e.keyset_aggregate_checked_batch_compressed(k, honest, hmsgs, dst),
        lambda e, k: e.keyset_aggregate_checked_batch(k, honest64, hmsgs, dst),
        lambda e, k: e.verify_batch_compressed(vp, vmsgs, bytes(vs), dst),
        lambda e, k: e.keyset_aggregate_checked_batch_compressed(k, wire, msgs, dst),
    ]

    def run(which):
        e = M.Engine(0)
        try:
            k = M.KeySet(e, com.pks, 70)
            try:
                return [steps[j](e, k) for j in which]
            finally:
                k.close()
        finally:
            e.close()

    fresh = [run([j])[0] for j in range(len(steps))]
    assert fresh[0][2] == bytes(3) and fresh[0][0] == compressed(eng, fresh[1][0]) and fresh[0][1:] == fresh[1][1:]
    assert fresh[2] == synth.bitmap_of([j not in (3, 9) for j in range(len(vk))])
    assert list(fresh[3][2]) == [0, 0, ST_SHORT, 0, 0, 0, ST_SHORT, ST_SHORT]
    got = run(range(len(steps)))
    for j, (a, b) in enumerate(zip(got, fresh)):
        assert a == b, "step %d differs from the same call on a context of its own" % j


def test_chain_on_wire_bytes(eng, W, wks):
    """two compressed collector outputs, concatenated, through the compressed per-committee merge and on to the compressed
    committee verify: every status-0 group sets its bit, a tampered byte clears it"""
    com = [0, 1, 1, 0]
    halves = []
    msgs = [b"wire chain %d" % g for g in range(len(com))]
    for h in range(2):
        pos_sets = [set(W.clean[c][(8 * h + g) % 3 + 12 * h:12 * h + 10]) for g, c in enumerate(com)]
        if h == 1:
            pos_sets[3] = set()                                          # the second collector has nothing for group 3
        wire = compress_entries(eng, W.sign(eng, com, pos_sets, msgs))
        halves.append(eng.keyset_committee_aggregate_checked_batch_compressed(wks, com, wire, msgs, W.dst))
    assert halves[0][2] == bytes(4) and halves[1][2] == bytes([0, 0, 0, ST_SHORT])
    groups = [[(h[1][g], h[0][32 * g:32 * g + 32]) for h in halves] for g in range(len(com))]
    out, rows, used, st = eng.keyset_committee_merge_checked_batch_compressed(wks, com, groups, msgs, W.dst)
    assert st == bytes(4) and used == [[True, True]] * 3 + [[True, False]]
    assert [r != h0 for r, h0 in zip(rows, halves[0][1])] == [True, True, True, False]
    bm = eng.keyset_committee_fast_aggregate_verify_batch_compressed(wks, com, rows, msgs, out, W.dst)
    assert bm == synth.bitmap_of([True] * 4)
    bad = bytearray(out); bad[32 * 2 + 31] ^= 1
    assert eng.keyset_committee_fast_aggregate_verify_batch_compressed(wks, com, rows, msgs, bytes(bad), W.dst) == synth.bitmap_of([True, True, False, True])


# ------------------------------------------------------------------ argument errors
class Harness:
    """one entry point with its default arguments (name -> value, in the C order; tuples become arrays) and its outputs,
    filled with 0x5a so that an error that touched one shows"""

    def __init__(self, lib, ctx, fn, args, outs):
        self.lib, self.ctx, self.fn, self.args, self.keep = lib, ctx, fn, args, []
        self.outs = {k: np.full(n, 0x5a, dtype=np.uint8) for k, n in outs.items()}

    def conv(self, v):
        if isinstance(v, tuple) and len(v) == 2 and isinstance(v[1], type):
            a = np.array(v[0], dtype=v[1]); self.keep.append(a)
            return a.ctypes.data_as({np.uint8: u8, np.uint32: u32, np.uint64: u64}[v[1]])
        if isinstance(v, int) and not isinstance(v, bool):
            return ctypes.c_size_t(v)
        return v

    def call(self, **over):
        vals = []
        for k, v in self.args.items():
            v = over.get(k, v)
            vals.append(self.outs[k].ctypes.data_as(u8) if v == "out" else self.conv(v))
        return getattr(self.lib, self.fn)(*vals)

    def untouched(self):
        return all(o.tobytes() == b"\x5a" * len(o) for o in self.outs.values())

    def err(self):
        return self.lib.blsbn254_last_error(self.ctx)


def test_argument_errors(eng, M, W):
    lib, ctx, dst = eng._lib, eng._ctx, b"TEST"
    coms = [list(range(13)), list(range(8, 24))]                         # rows of 2 bytes
    com13 = Committee(eng, 13, 95)                                       # (13 keys: no special ones)
    ks = M.KeySet(eng, com13.pks, 13)
    kc = M.KeySet(eng, W.reg.pks, W.n)
    bare = M.KeySet(eng, W.reg.pks, W.n)                                 # a handle without a committee table
    kc.set_committees(coms)
    e2 = M.Engine(0)
    sg = (list(bytes(32 * 4)), np.uint8)                                 # (the checks run before a signature is read)
    data = (list(b"abc"), np.uint8)
    U32, U64, U8 = np.uint32, np.uint64, np.uint8
    agg = Harness(lib, ctx, "blsbn254_keyset_aggregate_checked_batch_compressed", dict(
        c=ctx, k=ks._h, i=([0, 1, 12, 5], U32), s=sg, so=([0, 3, 4], U64), m=data, mo=([0, 1, 3], U64), g=2, d=dst, dl=4, o="out", r="out", t="out"),
        dict(o=64, r=4, t=2))
    cagg = Harness(lib, ctx, "blsbn254_keyset_committee_aggregate_checked_batch_compressed", dict(
        c=ctx, k=kc._h, cm=([0, 1], U32), p=([0, 1, 12, 5], U32), s=sg, so=([0, 3, 4], U64), m=data, mo=([0, 1, 3], U64), ro=([0, 2, 4], U64), g=2, d=dst, dl=4,
        o="out", r="out", t="out"), dict(o=64, r=4, t=2))
    mrg = Harness(lib, ctx, "blsbn254_keyset_merge_checked_batch_compressed", dict(
        c=ctx, k=ks._h, r=([3, 0, 0, 0x10, 0x20, 0], U8), s=sg, co=([0, 2, 3], U64), m=data, mo=([0, 1, 3], U64), g=2, d=dst, dl=4, o="out", q="out", u="out",
        t="out"), dict(o=64, q=4, u=1, t=2))
    cmrg = Harness(lib, ctx, "blsbn254_keyset_committee_merge_checked_batch_compressed", dict(
        c=ctx, k=kc._h, cm=([0, 1], U32), r=([3, 0, 0, 0x10, 0x20, 0], U8), ro=([0, 4, 6], U64), s=sg, co=([0, 2, 3], U64), m=data, mo=([0, 1, 3], U64),
        so=([0, 2, 4], U64), g=2, d=dst, dl=4, o="out", q="out", u="out", t="out"), dict(o=64, q=4, u=1, t=2))
    ver = Harness(lib, ctx, "blsbn254_keyset_committee_fast_aggregate_verify_batch_compressed", dict(
        c=ctx, k=kc._h, cm=([0, 1], U32), r=([3, 0x10, 0x20, 0], U8), ro=([0, 2, 4], U64), m=data, mo=([0, 1, 3], U64), s=sg, g=2, d=dst, dl=4, b="out"),
        dict(b=1))
    big = (1 << 23) + 1
    cases = {
        agg: [(dict(so=([0, 3, 2], U64)), b"offsets decrease"), (dict(mo=([0, 2, 1], U64)), b"offsets decrease"), (dict(so=([0, 3, big], U64)), b"2^23"),
              (dict(i=([0, 1, 13, 5], U32)), b"names no key"), (dict(i=([0, 1, 1, 5], U32)), b"strictly increase"), (dict(g=(1 << 22) + 1), b"launch chunk")],
        cagg: [(dict(k=bare._h), b"no committees"), (dict(cm=([0, 2], U32)), b"group 1 names committee 2 of 2"), (dict(p=([0, 1, 13, 5], U32)), b"entry 2 names no member"),
               (dict(p=([0, 1, 1, 5], U32)), b"strictly increase"), (dict(so=([0, 3, 2], U64)), b"offsets decrease"), (dict(mo=([0, 2, 1], U64)), b"offsets decrease"),
               (dict(ro=([0, 2, 1], U64)), b"offsets decrease"), (dict(ro=([0, 2, 3], U64)), b"group 1: the row must be 2 bytes"),
               (dict(so=([0, 3, big], U64)), b"2^23"), (dict(g=(1 << 22) + 1), b"launch chunk")],
        mrg: [(dict(co=([0, 3, 2], U64)), b"offsets decrease"), (dict(mo=([0, 2, 1], U64)), b"offsets decrease"), (dict(co=([0, 2, big + 2], U64)), b"2^23"),
              (dict(r=([3, 0xe0, 0, 0x10, 0x20, 0], U8)), b"contribution 0 sets a bit past the last key"), (dict(g=(1 << 22) + 1), b"launch chunk")],
        cmrg: [(dict(k=bare._h), b"no committees"), (dict(cm=([0, 2], U32)), b"group 1 names committee 2 of 2"),
               (dict(ro=([0, 4, 7], U64)), b"group 1: the contribution rows must be 1 x 2 bytes"), (dict(so=([0, 2, 3], U64)), b"group 1: the row must be 2 bytes"),
               (dict(r=([3, 0, 0, 0x30, 0x20, 0], U8)), b"contribution 1 sets a bit past the last member"), (dict(co=([0, 3, 2], U64)), b"offsets decrease"),
               (dict(ro=([0, 6, 4], U64)), b"offsets decrease"), (dict(mo=([0, 2, 1], U64)), b"offsets decrease"), (dict(so=([0, 4, 2], U64)), b"offsets decrease"),
               (dict(co=([0, 2, big + 2], U64), ro=([0, 4, 6 + (1 << 24)], U64)), b"2^23"), (dict(g=(1 << 22) + 1), b"launch chunk")],
        ver: [(dict(k=bare._h), b"no committees"), (dict(g=(1 << 22) + 1), b"launch chunk"), (dict(cm=([0, 2], U32)), b"committee 2"),
              (dict(r=([3, 0xe0, 0x20, 0], U8)), b"group 0")],
    }
    try:
        eng.profile_enable(True); eng.profile_reset()                    # every kernel launch of this context is recorded from here on
        for h, rows in cases.items():
            for name, v in h.args.items():
                if name in ("g", "dl") or (h is ver and name == "m"):    # (the verify calls take msgs == NULL for empty messages)
                    continue
                assert h.call(**{name: None}) == E_ARG and h.untouched(), (h.fn, name)
            assert h.call(c=e2._ctx) == E_ARG and h.untouched(), h.fn     # a key set that belongs to another context
            for over, text in rows:
                assert h.call(**over) == E_ARG and h.untouched(), (h.fn, over)
                assert text in h.err(), (h.fn, over, h.err())
            assert h.call(g=0) == 0 and h.untouched(), h.fn
        launched = eng.profile_read()
        eng.profile_enable(False); eng.profile_reset()
        assert launched == {}                                            # nothing was enqueued
        # after the errors the context still serves; offsets that do not start at 0 are only a base
        ent = sign_sets(eng, com13, [{0, 1, 12}, {5}], [b"a", b"bc"], dst)
        w = compress_entries(eng, ent)
        flat = b"".join(w[g][i] for g, s in enumerate(({0, 1, 12}, {5})) for i in sorted(s))
        assert agg.call(s=(list(flat), U8)) == 0 and agg.outs["t"].tobytes() == bytes(2)
        first = {k: o.tobytes() for k, o in agg.outs.items()}
        assert first["r"] == row_of({0, 1, 12}, 13) + row_of({5}, 13) and first["o"][32:] == w[1][5]
        for o in agg.outs.values():
            o[:] = 0x5a
        assert agg.call(i=([99, 0, 1, 12, 5], U32), s=(list(bytes(32) + flat), U8), so=([1, 4, 5], U64), m=(list(b"??abc"), U8), mo=([2, 3, 5], U64)) == 0
        assert {k: o.tobytes() for k, o in agg.outs.items()} == first
        with pytest.raises(ValueError):
            eng.keyset_aggregate_checked_batch_compressed(ks, [{0: ent[0][0]}], [b"a"], dst)          # 64 bytes where 32 are due
        with pytest.raises(ValueError):
            eng.keyset_merge_checked_batch_compressed(ks, [[([0], ent[0][0])]], [b"a"], dst)
        assert eng.keyset_aggregate_checked_batch_compressed(ks, [], [], dst) == (b"", b"", b"")
        assert eng.keyset_committee_merge_checked_batch_compressed(kc, [], [], [], dst) == (b"", [], [], b"")
    finally:
        eng.profile_enable(False)
        e2.close(); ks.close(); kc.close(); bare.close()
