"""CPU-only: the lane functions of the checked merge of partial aggregates per committee of a registered key set
(bls-bn254_amd/csrc/keyset_committee_merge.h over keyset_merge.h) compiled for the host with -DBN_CHECK, a wave run as 64 lane
states in lockstep with the votes formed by the harness, and the plain C++ of its host side (keyset_committee_merge_plan.h): the
ragged selection against a sequential Python model over committees of every width at which the code takes another path, with
launch cuts at several positions, the bytes a launch leaves alone, the argument walk, the layout prefixes and the repack of
failing groups.  A test tool; the product has no CPU path."""
import ctypes
import random

import numpy as np
import pytest

from tests import hostsim_build
from tests.helpers import bitmap, row_of, u32, u64

u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)
KCM_OK, KCM_OFF_DECREASE, KCM_TOO_MANY, KCM_ROWS_TOO_LARGE, KCM_COM_RANGE, KCM_ROW_SPAN, KCM_SEL_LEN, KCM_ROW_PAD = range(8)
USED, CAND = 1, 2
N_KEYS = 2200
# committees of 1, 31, 32, 33 and 65 members (1, 1, 1, 2, 3 words; rows of 1, 4, 4, 5, 9 bytes), one of 2050 members (65 words,
# 257-byte rows: the union lives in the merged row, lane 0 owns two words) and one of 2048 (64 words: the last width with the
# union in a register).  Listed in any order, overlapping: the selection never reads a member index
SIZES = [1, 31, 32, 33, 65, 2050, 2048]


def table():
    rnd = random.Random(1)
    return [rnd.sample(range(N_KEYS), s) for s in SIZES]


@pytest.fixture(scope="module")
def hs():
    so = hostsim_build.build("keyset_committee_merge_host.cpp", "libkeysetcommitteemergehost.so")
    lib = ctypes.CDLL(so)
    lib.hs_kcm_repack.restype = ctypes.c_size_t
    lib.hs_kcm_layout_contributions.restype = ctypes.c_size_t
    coms = table()
    members = u32([i for c in coms for i in c])
    off = u64(np.concatenate([[0], np.cumsum(SIZES)]))
    err = ctypes.create_string_buffer(256)
    assert lib.hs_kcm_table(members.ctypes.data_as(u32p), off.ctypes.data_as(u64p), ctypes.c_size_t(len(SIZES)), ctypes.c_size_t(N_KEYS), err) == 0, err.value
    wbase = (ctypes.c_uint32 * len(SIZES))()
    lib.hs_kcm_wbase(wbase)
    lib.wbase = list(wbase)
    assert lib.wbase == [int(x) for x in np.concatenate([[0], np.cumsum([(s + 31) // 32 for s in SIZES])])[:-1]]
    return lib


def rb_of(c):
    return (SIZES[c] + 7) // 8


def model_select(com, groups, sig_ok, mask, valid):
    """sequential: per contribution its byte, per group the union.  groups: lists of position sets; valid[c]: the valid positions"""
    flags, unions, s = [], [], 0
    for c, g in zip(com, groups):
        union = set()
        for pos in g:
            cand = bool(sig_ok[s]) and len(pos) > 0 and pos <= valid[c]
            used = cand and (mask is None or mask[s]) and not (pos & union)
            if used:
                union |= pos
            flags.append((CAND if cand else 0) | (USED if used else 0))
            s += 1
        unions.append(row_of(union, SIZES[c]))
    return flags, unions


def cvalid_words(hs, valid):
    total = sum((s + 31) // 32 for s in SIZES)
    words = [0] * total
    for c, ok in enumerate(valid):
        for j in ok:
            words[hs.wbase[c] + (j >> 5)] |= 1 << (j & 31)
    return u32(words)


def run_select(hs, com, groups, sig_ok, mask, valid, cuts, lead=0):
    """the call's rows behind `lead` bytes nobody reads; one launch per piece of `cuts`.  Returns flags, the merged rows, and
    whether every launch wrote exactly the bytes of its own groups' rows and flags"""
    rows = b"\x77" * lead + b"".join(row_of(p, SIZES[c]) for c, g in zip(com, groups) for p in g)
    ng = len(groups)
    goff = u32(np.concatenate([[0], np.cumsum([len(g) for g in groups])]))
    row_off = u64(lead + np.concatenate([[0], np.cumsum([len(g) * rb_of(c) for c, g in zip(com, groups)])]))
    sel_off = u64(1000 + np.concatenate([[0], np.cumsum([rb_of(c) for c in com])]))
    rbase, roff = (ctypes.c_uint64 * (ng + 1))(), (ctypes.c_uint64 * (ng + 1))()
    hs.hs_kcm_layout(row_off.ctypes.data_as(u64p), sel_off.ctypes.data_as(u64p), ctypes.c_size_t(ng), rbase, roff)
    assert list(rbase) == [int(x) - lead for x in row_off] and list(roff) == [int(x) - 1000 for x in sel_off]
    N, total = int(goff[-1]), int(roff[ng])
    cv, ca = cvalid_words(hs, valid), u32(com)
    flags = ctypes.create_string_buffer(b"\xee" * max(N, 1), max(N, 1))
    urows = ctypes.create_string_buffer(b"\xaa" * (total + 8), total + 8)   # every byte of every merged row must be written, none behind them
    edges = [0] + [c for c in cuts if 0 < c < ng] + [ng]
    own = True
    for lo, hi in zip(edges, edges[1:]):
        f1 = ctypes.create_string_buffer(b"\xee" * max(N, 1), max(N, 1))
        u1 = ctypes.create_string_buffer(b"\xaa" * (total + 8), total + 8)
        for f, u in ((flags, urows), (f1, u1)):
            hs.hs_kcm_select(rows[lead:] + b"\0", bytes(sig_ok) + b"\0", None if mask is None else bitmap(mask), goff.ctypes.data_as(u32p), ca.ctypes.data_as(u32p),
                             cv.ctypes.data_as(u32p), rbase, roff, lo, hi - lo, f, u)
        a, b = int(roff[lo]), int(roff[hi])
        own &= u1.raw[:a] == b"\xaa" * a and u1.raw[b:] == b"\xaa" * (total + 8 - b)
        own &= f1.raw[:int(goff[lo])] == b"\xee" * int(goff[lo]) and f1.raw[int(goff[hi]):N] == b"\xee" * (N - int(goff[hi]))
    assert urows.raw[total:] == b"\xaa" * 8
    return list(flags.raw[:N]), [urows.raw[int(roff[g]):int(roff[g + 1])] for g in range(ng)], own


def edge_positions(size):
    """the first and last position of the words at which lanes change hands"""
    W = (size + 31) // 32
    ws = sorted({w for w in (0, 1, 2, 62, 63, 64, W - 1) if w < W})
    return sorted({p for w in ws for p in (32 * w, min(32 * w + 31, size - 1))})


def selection_case(rnd):
    valid, com, groups = [], [], []
    for c, size in enumerate(SIZES):
        edge = edge_positions(size)
        invalid = {edge[-1], edge[len(edge) // 2]} if size > 1 else set()
        valid.append(set(range(size)) - invalid)
    for c, size in enumerate(SIZES):
        ok = sorted(valid[c])

        def some(k):
            return set(rnd.sample(ok, min(k, len(ok))))

        a = some(5)
        b = set([k for k in ok if k not in a][:3])
        mine = [
            [{k} for k in edge_positions(size) if k in valid[c]],             # disjoint single positions at every lane hand-over: all used
            [a, set(a), b, set()],                                              # a duplicate, a row beside them, an empty row
            [],                                                                 # no contribution
            [some(3) | (set(range(size)) - valid[c]), some(2)] if size > 1 else [set(), some(1)],      # a row on an invalid member
            [set(valid[c]), some(1)],                                           # every valid member, then anything overlaps
            [{ok[0], ok[-1]}, {ok[-1]}, {ok[len(ok) // 2]}, {ok[0]}],           # overlaps in the first and the last word
            [set(range(size))],                                                 # every member
            [some(rnd.randrange(0, 6)) for _ in range(rnd.randrange(1, 6))],
        ]
        com += [c] * len(mine); groups += mine
    order = list(range(len(com)))
    rnd.shuffle(order)                                                          # neighbours of every width beside one another
    return valid, [com[i] for i in order], [groups[i] for i in order]


def test_ragged_selection_against_the_model(hs):
    rnd = random.Random(941)
    valid, com, groups = selection_case(rnd)
    ng, N = len(groups), sum(len(g) for g in groups)
    assert sorted(set(com)) == list(range(len(SIZES))) and any(rb_of(c) % 4 for c in com)
    sig_sets = [[1] * N, [rnd.random() < 0.8 for _ in range(N)]]
    masks = [None, [True] * N, [False] * N, [rnd.random() < 0.6 for _ in range(N)]]
    for cuts, lead in (([], 0), ([1, 2, 5, ng - 1], 3), (list(range(1, ng)), 0), ([ng // 2], 1001)):
        for sig_ok in sig_sets:
            for mask in masks:
                want = model_select(com, groups, sig_ok, mask, valid)
                flags, unions, own = run_select(hs, com, groups, sig_ok, mask, valid, cuts, lead)
                assert (flags, unions) == want, (cuts, mask is None)
                assert own, "a launch wrote outside its own groups' rows or flags"
    # closed forms on the wide committee, all signatures good and no mask
    c, size = 5, SIZES[5]
    ok, edge = sorted(valid[c]), [k for k in edge_positions(size) if k in valid[c]]
    wide = [[{k} for k in edge], [set(valid[c]), {ok[3]}], [set(range(size))], [{ok[0], ok[-1]}, {ok[-1]}, {ok[1]}]]
    flags, unions, own = run_select(hs, [c] * 4, wide, [1] * (len(edge) + 6), None, valid, [2])
    assert flags == [CAND | USED] * len(edge) + [CAND | USED, CAND, 0, CAND | USED, CAND, CAND | USED] and own
    assert unions == [row_of(edge, size), row_of(valid[c], size), bytes(257), row_of({ok[0], ok[-1], ok[1]}, size)]


@pytest.mark.parametrize("c", range(len(SIZES)))
def test_admissible_once_an_earlier_one_is_masked_out(hs, c):
    """[A, B, C] with B overlapping A only and C overlapping B only: without a mask A and C are used; with A masked out B is
    used and C is not -- the fallback's second selection.  Between neighbours of another width"""
    size = SIZES[c]
    last = size - 1
    if size == 1:
        A, B, C = {0}, {0}, {0}
        want_plain, want_masked = [CAND | USED, CAND, CAND], [CAND, CAND | USED, CAND]
        u_plain, u_masked = {0}, {0}
    else:
        A, B, C = {0, last}, {last, 1}, {1, 2}
        want_plain, want_masked = [CAND | USED, CAND, CAND | USED], [CAND, CAND | USED, CAND]
        u_plain, u_masked = A | C, B
    valid = [set(range(s)) for s in SIZES]
    com = [4, c, 3]
    groups = [[{64}], [A, B, C], [{32}, {0, 32}]]
    tail = [CAND | USED, CAND]
    for cuts in ([], [1], [1, 2]):
        flags, unions, own = run_select(hs, com, groups, [1] * 6, None, valid, cuts)
        assert flags == [CAND | USED] + want_plain + tail and unions == [row_of({64}, 65), row_of(u_plain, size), row_of({32}, 33)] and own
        flags, unions, own = run_select(hs, com, groups, [1] * 6, [True, False, True, True, True, True], valid, cuts)
        assert flags == [CAND | USED] + want_masked + tail and unions[1] == row_of(u_masked, size) and own
        flags, unions, own = run_select(hs, com, groups, [1, 0, 1, 1, 1, 1], None, valid, cuts)      # the same through the signature byte
        assert flags == [CAND | USED, 0] + want_masked[1:] + tail and unions[1] == row_of(u_masked, size) and own


def walk(hs, com, rows, row_off, con_off, sel_off, max_con=1 << 23, max_bytes=1 << 30):
    where = (ctypes.c_uint64 * 3)()
    ng = len(com)
    code = hs.hs_kcm_walk(u32(com).ctypes.data_as(u32p), rows, u64(row_off).ctypes.data_as(u64p), u64(con_off).ctypes.data_as(u64p), u64(sel_off).ctypes.data_as(u64p),
                          ctypes.c_size_t(ng), ctypes.c_uint64(max_con), ctypes.c_uint64(max_bytes), where)
    return code, where[0], where[1], where[2]


def test_argument_walk(hs):
    # committees 1 (31 members, 4-byte rows, one padding bit), 3 (33 members, 5-byte rows, seven padding bits), 2 (32, none)
    com = [1, 3, 2]
    r1 = [row_of({0, 30}, 31), row_of(set(), 31)]
    r3 = [row_of({32}, 33)]
    r2 = [b"\xff" * 4, b"\xff" * 4]
    rows = b"".join(r1 + r3 + r2)
    ro, co, so = [0, 8, 13, 21], [0, 2, 3, 5], [0, 4, 9, 13]
    assert walk(hs, com, rows, ro, co, so)[0] == KCM_OK
    # no array needs to start at 0: the bytes before and behind the spans are not looked at
    assert walk(hs, com, b"\xff\xff" + rows + b"\xff", [2, 10, 15, 23], [7, 9, 10, 12], [100, 104, 109, 113])[0] == KCM_OK
    assert walk(hs, com, b"", [5, 5, 5, 5], [0, 0, 0, 0], so)[0] == KCM_OK                      # no contribution at all
    assert walk(hs, com, rows, ro, [0, 3, 2, 5], so)[:2] == (KCM_OFF_DECREASE, 1) and walk(hs, com, rows, ro, [0, 3, 2, 5], so)[3] == 0
    assert walk(hs, com, rows, [0, 8, 7, 21], co, so)[::3] == (KCM_OFF_DECREASE, 1)
    assert walk(hs, com, rows, ro, co, [0, 4, 9, 8])[::3] == (KCM_OFF_DECREASE, 2)
    assert walk(hs, com, rows, ro, [0, 3, 2, 5], so, max_con=0)[0] == KCM_OFF_DECREASE           # the offsets come first
    assert walk(hs, com, rows, ro, co, so, max_con=4)[0] == KCM_TOO_MANY and walk(hs, com, rows, ro, co, so, max_con=5)[0] == KCM_OK
    assert walk(hs, com, rows, ro, co, so, max_bytes=20)[0] == KCM_ROWS_TOO_LARGE and walk(hs, com, rows, ro, co, so, max_bytes=21)[0] == KCM_OK
    assert walk(hs, [1, 7, 2], rows, ro, co, so)[:2] == (KCM_COM_RANGE, 1)
    assert walk(hs, com, rows, [0, 8, 12, 20], co, so)[:2] == (KCM_ROW_SPAN, 1)                  # 4 bytes for one row of 5
    assert walk(hs, com, rows, [0, 7, 12, 20], co, so)[:2] == (KCM_ROW_SPAN, 0)
    assert walk(hs, com, rows, ro, [0, 2, 3, 4], so)[:2] == (KCM_ROW_SPAN, 2)                    # 8 bytes for one row of 4
    assert walk(hs, com, rows, ro, co, [0, 4, 8, 12])[:2] == (KCM_SEL_LEN, 1)
    assert walk(hs, com, rows, ro, co, [0, 5, 10, 14])[:2] == (KCM_SEL_LEN, 0)
    pad1 = r1[0] + bytes([0, 0, 0, 0x80])                                                        # position 31 of 31 members
    assert walk(hs, com, pad1 + b"".join(r3 + r2), ro, co, so)[:3] == (KCM_ROW_PAD, 0, 1)
    pad3 = bytes([0, 0, 0, 0, 2])                                                                # position 33 of 33 members
    assert walk(hs, com, b"".join(r1) + pad3 + b"".join(r2), ro, co, so)[:3] == (KCM_ROW_PAD, 1, 2)
    assert walk(hs, com, b"".join(r1) + pad3 + b"".join(r2), ro, [10, 12, 13, 15], so)[:3] == (KCM_ROW_PAD, 1, 12)   # as con_off counts


def test_layout_of_contributions(hs):
    com = [3, 0, 5, 1, 4]
    con_off = u64([4, 6, 6, 7, 10, 11])                                  # an empty group, offsets that do not start at 0
    ccom, coff = (ctypes.c_uint32 * 7)(), (ctypes.c_uint64 * 8)()
    n = hs.hs_kcm_layout_contributions(u32(com).ctypes.data_as(u32p), con_off.ctypes.data_as(u64p), ctypes.c_size_t(5), ccom, coff)
    assert n == 7 and list(ccom) == [3, 3, 5, 1, 1, 1, 4]
    assert list(coff) == [0, 5, 10, 267, 271, 275, 279, 288]


def test_repack_of_failing_groups(hs):
    rnd = random.Random(7)
    com = [3, 1, 5, 0, 4]
    sizes = [3, 1, 0, 4, 2]
    lead, lead_bytes = 2, 11                                             # the call's offsets do not start at 0
    N = lead + sum(sizes)
    con_off = u64(lead + np.concatenate([[0], np.cumsum(sizes)]))
    row_off = u64(lead_bytes + np.concatenate([[0], np.cumsum([k * rb_of(c) for c, k in zip(com, sizes)])]))
    rows = bytes(rnd.randrange(256) for _ in range(int(row_off[-1]) + 3))
    sigs = [bytes(rnd.randrange(256) for _ in range(64)) for _ in range(N)]
    cand = [1, 0, 1, 1, 0, 1, 1, 1, 0, 0]                                # by contribution of the call, from its first one

    def row_at(g, i):
        a = int(row_off[g]) + i * rb_of(com[g])
        return rows[a:a + rb_of(com[g])]

    for fail in ([0, 3], [3], [1, 2, 4], [0, 1, 2, 3, 4], []):
        nf = len(fail)
        co, po = (ctypes.c_uint32 * max(nf, 1))(), (ctypes.c_uint64 * N)()
        oo, rr, ss = ((ctypes.c_uint64 * (nf + 1))() for _ in range(3))
        ro, so = ctypes.create_string_buffer(len(rows)), ctypes.create_string_buffer(N * 64)
        cnt = hs.hs_kcm_repack(u64(fail).ctypes.data_as(u64p), ctypes.c_size_t(nf), u32(com).ctypes.data_as(u32p), rows, row_off.ctypes.data_as(u64p), b"".join(sigs),
                               con_off.ctypes.data_as(u64p), bitmap(cand), co, po, oo, rr, ss, ro, so)
        want_pos, want_off, want_roff, want_sel, want_rows = [], [0], [0], [0], b""
        for g in fail:
            keep = [s for s in range(int(con_off[g]), int(con_off[g + 1])) if cand[s - lead]]
            want_pos += keep
            want_rows += b"".join(row_at(g, s - int(con_off[g])) for s in keep)
            want_off.append(len(want_pos)); want_roff.append(len(want_rows)); want_sel.append(want_sel[-1] + rb_of(com[g]))
        assert cnt == len(want_pos) and list(po)[:cnt] == want_pos and list(co)[:nf] == [com[g] for g in fail], fail
        assert list(oo) == want_off and list(rr) == want_roff and list(ss) == want_sel, fail
        assert ro.raw[:len(want_rows)] == want_rows and so.raw[:cnt * 64] == b"".join(sigs[p] for p in want_pos)
