"""CPU-only: the lane functions of the checked signature aggregation per committee of a registered key set
(bls-bn254_amd/csrc/keyset_committee_agg.h) compiled for the host with -DBN_CHECK, and the plain C++ of its host side
(keyset_committee_agg_plan.h): the argument walk, the repack of failing groups, the group search of the scan, the ragged rows
and the whole optimistic selection against a Python model, each over launch cuts at several positions.  A test tool; the product
has no CPU path."""
import ctypes
import random

import numpy as np
import pytest

from tests import hostsim_build
from tests.helpers import b32, bitmap, launches, model_candidate, u32, u64
from tests.keyset_support import words

u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)
KCA_OK, KCA_OFF_DECREASE, KCA_TOO_MANY, KCA_COM_RANGE, KCA_ROW_LEN, KCA_POS_RANGE, KCA_POS_ORDER = range(7)
N_KEYS = 200
# committees of 1, 31, 32, 33 and 65 members over 200 keys: 1 and 2 overlap, 3 is listed in descending order, 4 is a shuffle
COMS = [[77], list(range(10, 41)), list(range(30, 62)), list(range(132, 99, -1)), random.Random(3).sample(range(N_KEYS), 65)]
SIZES = [len(c) for c in COMS]
assert SIZES == [1, 31, 32, 33, 65]


def rb(size):
    return (size + 7) // 8


@pytest.fixture(scope="module")
def hs():
    so = hostsim_build.build("keyset_committee_aggregate_host.cpp", "libkeysetcommitteeaggregatehost.so")
    lib = ctypes.CDLL(so)
    lib.hs_kca_repack.restype = ctypes.c_size_t
    members = u32([i for c in COMS for i in c])
    off = u64(np.cumsum([0] + SIZES))
    err = ctypes.create_string_buffer(256)
    assert lib.hs_kca_table(members.ctypes.data_as(u32p), off.ctypes.data_as(u64p), ctypes.c_size_t(len(COMS)), ctypes.c_size_t(N_KEYS), err) == 0, err.value
    coms = (ctypes.c_uint32 * (4 * len(COMS)))()
    lib.hs_kca_coms(coms)
    wb = np.cumsum([0] + [words(s) for s in SIZES])
    assert [tuple(coms[4 * c:4 * c + 3]) for c in range(len(COMS))] == [(int(off[c]), SIZES[c], int(wb[c])) for c in range(len(COMS))]
    lib.members, lib.wbase = members, [int(x) for x in wb]
    return lib


def sel_offsets(com, lead=0):
    return u64(lead + np.cumsum([0] + [rb(SIZES[c]) for c in com]))


def walk(hs, com, pos, sig_off, sel_off, max_entries=1 << 23):
    where = (ctypes.c_uint64 * 2)()
    com, pos, sig_off, sel_off = u32(com), u32(pos if len(pos) else [0]), u64(sig_off), u64(sel_off)
    code = hs.hs_kca_walk(com.ctypes.data_as(u32p), pos.ctypes.data_as(u32p), sig_off.ctypes.data_as(u64p), sel_off.ctypes.data_as(u64p),
                          ctypes.c_size_t(len(com)), ctypes.c_uint64(max_entries), where)
    return code, where[0], where[1]


def test_argument_walk(hs):
    com = [1, 4, 0]
    so = sel_offsets(com)
    assert list(so) == [0, 4, 13, 14]
    assert walk(hs, com, [0, 5, 30, 64, 0], [0, 3, 4, 5], so)[0] == KCA_OK              # the first and the last position of a committee
    assert walk(hs, com, [], [0, 0, 0, 0], so)[0] == KCA_OK
    assert walk(hs, [4, 4], [5, 4, 3, 3], [0, 1, 2], sel_offsets([4, 4]))[0] == KCA_OK  # order is per group, not across groups
    # offsets that do not start at 0: the entries before the first offset are not looked at, the rows are measured by differences
    assert walk(hs, com, [99, 99, 0, 5, 30, 64, 0], [2, 5, 6, 7], sel_offsets(com, lead=1000))[0] == KCA_OK
    assert walk(hs, com, [99, 99, 0, 5, 31, 64, 0], [2, 5, 6, 7], sel_offsets(com, lead=1000)) == (KCA_POS_RANGE, 0, 4)
    # every refusal
    assert walk(hs, com, [0, 1], [0, 2, 1, 2], so)[:2] == (KCA_OFF_DECREASE, 1)
    assert walk(hs, com, [0, 1, 2], [0, 3, 3, 3], so, max_entries=2)[0] == KCA_TOO_MANY
    assert walk(hs, com, [0, 1, 2], [0, 3, 3, 3], so, max_entries=3)[0] == KCA_OK
    assert walk(hs, [1, 5, 0], [0], [0, 1, 1, 1], so)[:2] == (KCA_COM_RANGE, 1)         # com[g] == n_com
    assert walk(hs, com, [0, 31], [0, 2, 2, 2], so) == (KCA_POS_RANGE, 0, 1)            # pos == size
    assert walk(hs, com, [0, 0, 1], [0, 1, 1, 3], so) == (KCA_POS_RANGE, 2, 2)          # position 1 of a committee of one
    assert walk(hs, com, [1, 4, 4], [0, 3, 3, 3], so) == (KCA_POS_ORDER, 0, 2)          # equal neighbours
    assert walk(hs, com, [1, 2, 6, 5], [0, 2, 4, 4], so) == (KCA_POS_ORDER, 1, 3)       # decreasing
    assert walk(hs, com, [], [0, 0, 0, 0], [0, 4, 12, 13])[:2] == (KCA_ROW_LEN, 1)      # 8 bytes for 65 members
    assert walk(hs, com, [], [0, 0, 0, 0], [0, 4, 14, 15])[:2] == (KCA_ROW_LEN, 1)      # 10 bytes
    assert walk(hs, com, [], [0, 0, 0, 0], [0, 4, 13, 13])[:2] == (KCA_ROW_LEN, 2)      # an empty row
    assert walk(hs, com, [], [0, 0, 0, 0], [4, 0, 9, 10])[:2] == (KCA_ROW_LEN, 0)       # decreasing row offsets
    # the committee is checked before the row, the row before the positions
    assert walk(hs, [9, 4, 0], [70], [0, 1, 1, 1], [0, 1, 2, 3])[:2] == (KCA_COM_RANGE, 0)
    assert walk(hs, com, [70], [0, 1, 1, 1], [0, 5, 14, 15])[:2] == (KCA_ROW_LEN, 0)


def test_layout(hs):
    com = [4, 0, 3, 1, 2, 4]
    for lead in (0, 37):
        so = sel_offsets(com, lead)
        wpre, roff = (ctypes.c_uint64 * 7)(), (ctypes.c_uint64 * 7)()
        c = u32(com)
        hs.hs_kca_layout(c.ctypes.data_as(u32p), so.ctypes.data_as(u64p), ctypes.c_size_t(6), wpre, roff)
        assert list(wpre) == [0, 3, 4, 6, 7, 8, 11]
        assert list(roff) == [0, 9, 10, 15, 19, 23, 32]


def test_repack_of_failing_groups(hs):
    com = [4, 0, 3, 1, 4]
    groups = [[0, 31, 32, 64], [0], [], [1, 2, 29, 30], [8, 9]]
    cand = [[1, 0, 1, 1], [1], [], [0, 1, 1, 1], [0, 0]]
    lead, sel_lead = 2, 11                                              # neither the entry offsets nor the row offsets start at 0
    pos = u32([99, 99] + [p for g in groups for p in g])
    off = u64(lead + np.cumsum([0] + [len(g) for g in groups]))
    so = sel_offsets(com, sel_lead)
    rows = bytearray(int(so[-1] - so[0]))
    for g, (ps, cs) in enumerate(zip(groups, cand)):
        for p, c in zip(ps, cs):
            if c:
                rows[int(so[g]) - sel_lead + (p >> 3)] |= 1 << (p & 7)
    cm = u32(com)
    for fail in ([0, 3], [3], [1, 2, 4], [0, 1, 2, 3, 4], []):
        n, nf = len(pos), len(fail)
        co, po, sr = (ctypes.c_uint32 * max(nf, 1))(), (ctypes.c_uint32 * n)(), (ctypes.c_uint64 * n)()
        oo, so_out = (ctypes.c_uint64 * (nf + 1))(), (ctypes.c_uint64 * (nf + 1))()
        f = u64(fail if fail else [0])
        cnt = hs.hs_kca_repack(f.ctypes.data_as(u64p), ctypes.c_size_t(nf), cm.ctypes.data_as(u32p), pos.ctypes.data_as(u32p), off.ctypes.data_as(u64p),
                               so.ctypes.data_as(u64p), bytes(rows), co, po, sr, oo, so_out)
        want_pos, want_src, want_off, want_sel = [], [], [0], [0]
        for g in fail:
            for j, (p, c) in enumerate(zip(groups[g], cand[g])):
                if c:
                    want_pos.append(p); want_src.append(int(off[g]) + j)
            want_off.append(len(want_pos)); want_sel.append(want_sel[-1] + rb(SIZES[com[g]]))
        assert cnt == len(want_pos) and list(po)[:cnt] == want_pos and list(sr)[:cnt] == want_src, fail
        assert list(oo) == want_off and list(so_out) == want_sel and list(co)[:nf] == [com[g] for g in fail], fail
        assert all(int(pos[s]) == p for s, p in zip(want_src, want_pos))


def model_group(goff, s):
    return max(g for g in range(len(goff) - 1) if goff[g] <= s)


@pytest.mark.parametrize("lens", [[0, 0, 3, 1], [2, 0, 0, 0, 5, 0, 1], [4, 1, 0, 0], [0, 1, 0], [7], [0, 0, 2, 0, 0, 3, 0, 0]])
def test_group_search_with_empty_groups(hs, lens):
    goff = u32(np.cumsum([0] + lens))
    n, ng = int(goff[-1]), len(lens)
    want = [model_group(list(goff), s) for s in range(n)]
    assert all(lens[g] > 0 for g in want)
    for cuts in ([], [1], [2, 3], list(range(1, n))):
        got = []
        for lo, hi in launches(n, cuts):
            out = (ctypes.c_uint32 * (hi - lo))()
            hs.hs_kca_groups(goff.ctypes.data_as(u32p), ng, lo, hi - lo, out)
            got += list(out)
        assert got == want, (lens, cuts)


class Case:
    """groups over the committees above in an order that interleaves them, with empty groups at the front, in the middle and at
    the end, full groups and groups that touch the first and last position of every word"""

    def __init__(self, seed):
        rnd = random.Random(seed)
        self.com = [2, 4, 0, 3, 1, 4, 0, 3, 2, 1, 4, 3]
        edge = lambda s: sorted({0, s - 1} | {p for p in (31, 32, 63, 64) if p < s})
        pick = [[], None, [0], "edge", "full", "edge", [], "full", "edge", None, "full", []]
        self.groups = []
        for c, p in zip(self.com, pick):
            s = SIZES[c]
            self.groups.append(list(range(s)) if p == "full" else edge(s) if p == "edge" else sorted(rnd.sample(range(s), s // 2)) if p is None else p)
        self.pos = u32([p for g in self.groups for p in g] or [0])
        self.goff = u32(np.cumsum([0] + [len(g) for g in self.groups]))
        self.n, self.ng = int(self.goff[-1]), len(self.com)
        self.sel_off = sel_offsets(self.com)
        self.wpre = u64(np.cumsum([0] + [words(SIZES[c]) for c in self.com]))
        self.roff = u64(self.sel_off - self.sel_off[0])
        self.cm = u32(self.com)


def rows_of(hs, case, cand, cuts, only=None):
    """the rows buffer with 8 guard bytes on either side, every byte 0xaa before the launches"""
    total = int(case.roff[-1])
    buf = ctypes.create_string_buffer(b"\xaa" * (total + 16), total + 16)
    base = ctypes.cast(ctypes.byref(buf, 8), u8p)
    pieces = launches(int(case.wpre[-1]), cuts) if only is None else [only]
    for lo, hi in pieces:
        hs.hs_kca_rows(case.pos.ctypes.data_as(u32p), bitmap(cand), case.goff.ctypes.data_as(u32p), case.wpre.ctypes.data_as(u64p), case.roff.ctypes.data_as(u64p),
                       case.cm.ctypes.data_as(u32p), case.ng, ctypes.c_uint64(lo), hi - lo, base)
    raw = buf.raw
    return raw[:8], [raw[8 + int(case.roff[g]):8 + int(case.roff[g + 1])] for g in range(case.ng)], raw[8 + total:]


def model_rows(case, cand):
    out, s = [], 0
    for g, ps in enumerate(case.groups):
        r = bytearray(rb(SIZES[case.com[g]]))
        for p in ps:
            if cand[s]:
                r[p >> 3] |= 1 << (p & 7)
            s += 1
        out.append(bytes(r))
    return out


@pytest.mark.parametrize("cuts", [[], [4], [1, 2, 3], [5, 7, 11, 13], list(range(1, 21))])
def test_ragged_rows(hs, cuts):
    case = Case(17)
    assert int(case.wpre[-1]) == 21 and {len(r) for r in model_rows(case, [0] * case.n)} == {1, 4, 5, 9}
    rnd = random.Random(19)
    for name, cand in (("ones", [True] * case.n), ("zeros", [False] * case.n), ("random", [rnd.random() < 0.6 for _ in range(case.n)])):
        before, got, after = rows_of(hs, case, cand, cuts)
        assert got == model_rows(case, cand), (name, cuts)               # every byte of every row is written, an empty group's zero row too
        assert before == b"\xaa" * 8 and after == b"\xaa" * 8
    before, got, after = rows_of(hs, case, [True] * case.n, cuts)
    # closed forms: the padding bits of the last byte are 0 in a full row of 31, 33, 65 members and of 1
    full = {1: b"\x01", 31: b"\xff\xff\xff\x7f", 32: b"\xff" * 4, 33: b"\xff" * 4 + b"\x01", 65: b"\xff" * 8 + b"\x01"}
    for g, ps in enumerate(case.groups):
        size = SIZES[case.com[g]]
        if len(ps) == size:
            assert got[g] == full[size], g
        if not ps:
            assert got[g] == bytes(rb(size)), g


def test_rows_leave_their_neighbours_alone(hs):
    """the lanes of ONE group write that group's row and not a byte of the rows next to it (rows are unaligned and their last
    word is partial)"""
    case = Case(17)
    cand = [True] * case.n
    want = model_rows(case, cand)
    for g in range(case.ng):
        before, got, after = rows_of(hs, case, cand, [], only=(int(case.wpre[g]), int(case.wpre[g + 1])))
        assert got[g] == want[g], g
        assert all(got[h] == b"\xaa" * len(got[h]) for h in range(case.ng) if h != g), g
        assert before == b"\xaa" * 8 and after == b"\xaa" * 8


def test_descending_committee_resolves_through_the_member_list(hs):
    case = Case(17)
    want = [COMS[case.com[g]][p] for g, ps in enumerate(case.groups) for p in ps]
    for cuts in ([], [3], [8, 9], list(range(1, case.n))):
        idx = (ctypes.c_uint32 * case.n)()
        for lo, hi in launches(case.n, cuts):
            hs.hs_kca_resolve(hs.members.ctypes.data_as(u32p), case.cm.ctypes.data_as(u32p), case.goff.ctypes.data_as(u32p), case.ng, case.pos.ctypes.data_as(u32p),
                              lo, hi - lo, idx)
        assert list(idx) == want, cuts
    g3 = case.com.index(3)
    assert COMS[3][0] == 132 and want[int(case.goff[g3])] == 132 - case.groups[g3][0]


def cvalid_words(key_valid):
    out = []
    for mem in COMS:
        for w in range(words(len(mem))):
            out.append(sum(key_valid[i] << j for j, i in enumerate(mem[32 * w:32 * w + 32])))
    return u32(out)


def test_optimistic_selection_against_the_model(hs, oracle, pyref):
    """scan + rows, given the keys' validity bits and signatures of every shape: the candidate bit of an entry is (validity bit of
    members[position]) AND (the signature is a usable point) AND (the mask bit), and the row has exactly the candidates' bits"""
    from tests import synth
    P = synth.P
    G = oracle.g1_generator()
    pts = [oracle.g1_mul(G, k) for k in (1, 2, 12345, pyref.R - 1)]
    off = bytearray(pts[1]); off[63] ^= 1
    shapes = pts + [bytes(off), b32(P) + pts[0][32:], pts[0][:32] + b32(P + 1), bytes(32) + b32(1), bytes(64), b"\xff" * 64]
    usable = [int(model_candidate(s, P)) for s in shapes]
    assert usable == [1, 1, 1, 1, 0, 0, 0, 0, 0, 0]
    case = Case(23)
    rnd = random.Random(29)
    kind = [rnd.randrange(len(shapes)) if rnd.random() < 0.3 else rnd.randrange(4) for _ in range(case.n)]
    sigs = b"".join(shapes[k] for k in kind)
    some_valid = [int(rnd.random() < 0.7) for _ in range(N_KEYS)]
    key_of = [COMS[case.com[g]][p] for g, ps in enumerate(case.groups) for p in ps]
    masks = [None, [True] * case.n, [rnd.random() < 0.5 for _ in range(case.n)]]
    seen = set()
    for cuts in ([], [8], [5, 6, 40], list(range(8, case.n, 8))):
        for key_valid in ([1] * N_KEYS, some_valid, [0] * N_KEYS):
            cv = cvalid_words(key_valid)
            for mask in masks:
                want = [int(usable[kind[s]] and key_valid[key_of[s]] and (mask is None or mask[s])) for s in range(case.n)]
                cand, ident = [], []
                for lo, hi in launches(case.n, cuts):
                    c = ctypes.create_string_buffer(hi - lo); z = ctypes.create_string_buffer(hi - lo)
                    hs.hs_kca_scan(cv.ctypes.data_as(u32p), case.cm.ctypes.data_as(u32p), case.goff.ctypes.data_as(u32p), case.ng, case.pos.ctypes.data_as(u32p), sigs,
                                   None if mask is None else bitmap(mask), lo, hi - lo, c, z)
                    cand += list(c.raw); ident += list(z.raw)
                assert cand == want, (cuts, mask is None)
                assert ident == [1 - c for c in want], "a non-candidate is stored as the identity, a candidate as its point"
                _, rows, _ = rows_of(hs, case, cand, [3, 10])
                assert rows == model_rows(case, want)
                seen.add(sum(want))
    assert len(seen) > 3 and 0 in seen
