"""CPU-only: the host-side planners of the segmented reductions over ragged groups (bls-bn254_amd/csrc/seg_plan.h), the very
header the library compiles, against a model written here and against the properties every plan must have: which items a
launch takes, which groups it serves, and the (start, len) run descriptors of every level.  The start of an empty run is not
compared: no kernel reads an item of one."""
import ctypes
import random

import numpy as np
import pytest

from tests import hostsim_build

T_BIG = 4096                # the library's hand-over size (host_threshold_batch.hip)
SIZES = (0, 1, 2, 3, 7, 8, 9, 16, 17, 40, 100)
NAMED = ([0], [0, 0, 0], [1], [8, 8], [9, 0, 7], [3, 100, 0, 2], [100], [5, 0, 0])


@pytest.fixture(scope="module")
def hs():
    so = hostsim_build.build("seg_plan_host.cpp", "libsegplanhost.so")
    lib = ctypes.CDLL(so)
    for f in (lib.hs_seg_levels, lib.hs_seg_cut, lib.hs_seg_whole):
        f.restype = ctypes.c_long
    lib.hs_seg_levels.argtypes = [ctypes.c_void_p] + [ctypes.c_size_t] * 2
    lib.hs_seg_cut.argtypes = [ctypes.c_void_p] + [ctypes.c_size_t] * 3
    lib.hs_seg_whole.argtypes = [ctypes.c_void_p] + [ctypes.c_size_t] * 4
    lib.hs_seg_descriptors.restype = ctypes.c_size_t
    lib.hs_seg_read.argtypes = [ctypes.c_void_p] * 3
    return lib


def offsets_list(sizes):
    return [0] + [int(x) for x in np.cumsum(sizes)]


def read_plan(hs, words):
    """-> start, len, {items_max, m_max, launches: [{lo, hi, ga, gb, carry, levels: [(first, count)]}]}"""
    assert words >= 3, "the planner reports no convergence"
    nd = hs.hs_seg_descriptors()
    start, ln, flat = np.zeros(nd, np.uint32), np.zeros(nd, np.uint32), np.zeros(words, np.uint64)
    hs.hs_seg_read(start.ctypes.data, ln.ctypes.data, flat.ctypes.data)
    flat = [int(x) for x in flat]
    plan = {"items_max": flat[0], "m_max": flat[1], "launches": []}
    p = 3
    for _ in range(flat[2]):
        lo, hi, ga, gb, carry, nl = flat[p:p + 6]
        p += 6
        plan["launches"].append({"lo": lo, "hi": hi, "ga": ga, "gb": gb, "carry": bool(carry), "levels": [(flat[p + 2 * k], flat[p + 2 * k + 1]) for k in range(nl)]})
        p += 2 * nl
    assert p == words
    return [int(x) for x in start], [int(x) for x in ln], plan


def run_levels(hs, ranges, G):
    a = np.array(ranges, np.uint64).reshape(-1)
    return read_plan(hs, hs.hs_seg_levels(a.ctypes.data, len(ranges), G))


def run_cut(hs, rel, chunk, G):
    a = np.array(rel, np.uint64)
    return read_plan(hs, hs.hs_seg_cut(a.ctypes.data, len(rel) - 1, chunk, G))


def run_whole(hs, rel, chunk, G, t_big):
    a = np.array(rel, np.uint32)
    return read_plan(hs, hs.hs_seg_whole(a.ctypes.data, len(rel) - 1, chunk, G, t_big))


# ------------------------------------------------------------------ the model
def model_levels(ranges, G, start, ln):
    """appends the descriptors of every level for segments `ranges` -> [(first, count)]"""
    levels, cur = [], list(ranges)
    while True:
        first, nxt = len(start), []
        for a, b in cur:
            p = len(start) - first
            if a == b:
                start.append(a)
                ln.append(0)
            for s in range(a, b, G):
                start.append(s)
                ln.append(min(G, b - s))
            nxt.append((p, len(start) - first))
        levels.append((first, len(start) - first))
        if levels[-1][1] == len(cur):
            return levels
        cur = nxt


def items_max_of(launches):
    return max([1] + [cnt for L in launches for _, cnt in L["levels"][:-1]])


def cut_ranges(rel, L):
    """group g of launch L holds the items of the group that lie in the launch, launch-local"""
    clamp = lambda x: min(max(x, L["lo"]), L["hi"]) - L["lo"]
    return [(clamp(rel[g]), clamp(rel[g + 1])) for g in range(L["ga"], L["gb"])]


def whole_ranges(rel, L, t_big):
    return [(0, 0) if rel[g + 1] - rel[g] > t_big else (rel[g] - L["lo"], rel[g + 1] - L["lo"]) for g in range(L["ga"], L["gb"])]


def model_cut(rel, chunk, G):
    ng, N = len(rel) - 1, rel[-1]
    start, ln, launches, lo, g = [], [], [], 0, 0
    while True:
        lim = min(N, lo + chunk)
        inside = [r for r in rel if lo < r <= lim]
        hi = max(inside) if inside else lim
        gb = ng if hi == N else min(i for i in range(ng + 1) if rel[i] >= hi)
        L = {"lo": lo, "hi": hi, "ga": g, "gb": gb, "carry": rel[g] < lo}
        L["levels"] = model_levels(cut_ranges(rel, L), G, start, ln)
        launches.append(L)
        g = gb - 1 if gb > g and rel[gb] > hi else gb
        lo = hi
        if lo >= N:
            return start, ln, {"items_max": items_max_of(launches), "m_max": 0, "launches": launches}


def model_whole(rel, chunk, G, t_big):
    ng, N = len(rel) - 1, rel[-1]
    big = lambda g: rel[g + 1] - rel[g] > t_big
    start, ln, launches, lo, g = [], [], [], 0, 0
    while g < ng:
        lim = min(N, lo + chunk)
        hi, gb, cut = lo, g, False
        while gb < ng:
            b = rel[gb + 1]
            if b <= lim or (hi == lo and not big(gb)):      # a whole group; the launch's first one whatever its size
                hi, gb = b, gb + 1
                if b > lim:
                    break
            else:
                if big(gb) and lim > hi:                    # a hand-over group may be cut anywhere
                    hi, cut = lim, True
                break
        L = {"lo": lo, "hi": hi, "ga": g, "gb": gb + (1 if cut else 0), "carry": False}
        L["levels"] = model_levels(whole_ranges(rel, L, t_big), G, start, ln)
        launches.append(L)
        g, lo = gb, hi
    return start, ln, {"items_max": items_max_of(launches), "m_max": max(L["hi"] - L["lo"] for L in launches), "launches": launches}


def assert_same(got, want):
    (gs, gl, gp), (ws, wl, wp) = got, want
    assert gp == wp
    assert gl == wl
    assert [s for s, n in zip(gs, gl) if n] == [s for s, n in zip(ws, wl) if n]      # an empty run's start is free


# ------------------------------------------------------------------ the properties
def check_levels(ranges, G, start, ln, levels):
    segs = list(ranges)
    for first, count in levels:
        pos, nxt = first, []
        for a, b in segs:
            p0 = pos
            if a == b:                                      # an empty segment: exactly one run of length 0
                assert ln[pos] == 0
                pos += 1
            s = a
            while s < b:                                    # the runs partition the segment's items, in order
                assert start[pos] == s and 1 <= ln[pos] <= G and s + ln[pos] <= b
                s += ln[pos]
                pos += 1
            nxt.append((p0 - first, pos - first))
        assert pos == first + count
        segs = nxt                                          # the runs are the next level's items
    assert levels[-1][1] == len(ranges)                     # one run per segment


def check_tiling(launches, N):
    assert launches[0]["lo"] == 0 and launches[-1]["hi"] == N
    assert all(a["hi"] == b["lo"] for a, b in zip(launches, launches[1:]))


def check_cut(rel, chunk, G, start, ln, plan):
    ng, N, launches = len(rel) - 1, rel[-1], plan["launches"]
    check_tiling(launches, N)
    seen = set()
    for L in launches:
        lo, hi = L["lo"], L["hi"]
        assert hi - lo <= chunk
        inside = [r for r in rel if lo < r <= min(N, lo + chunk)]
        if inside:
            assert hi == max(inside)
        assert L["carry"] == (rel[L["ga"]] < lo)
        seen.update(range(L["ga"], L["gb"]))
        check_levels(cut_ranges(rel, L), G, start, ln, L["levels"])
    assert seen == set(range(ng))
    if N == 0:
        assert len(launches) == 1 and (launches[0]["ga"], launches[0]["gb"]) == (0, ng)
    assert plan["items_max"] == items_max_of(launches)


def check_whole(rel, chunk, G, t_big, start, ln, plan):
    ng, N, launches = len(rel) - 1, rel[-1], plan["launches"]
    check_tiling(launches, N)
    for g in range(ng):
        a, b = rel[g], rel[g + 1]
        holders = [L for L in launches if L["ga"] <= g < L["gb"]]
        if b - a <= t_big:                                  # in exactly one launch, wholly
            assert len(holders) == 1 and holders[0]["lo"] <= a and b <= holders[0]["hi"]
        else:                                               # in every launch it overlaps, as ONE empty run
            assert all(L in holders for L in launches if max(a, L["lo"]) < min(b, L["hi"]))
            for L in holders:
                first = L["levels"][0][0]
                e = g - L["ga"]
                runs = sum(max(1, -(-(y - x) // G)) for x, y in whole_ranges(rel, L, t_big)[:e])
                assert ln[first + runs] == 0
    for L in launches:
        check_levels(whole_ranges(rel, L, t_big), G, start, ln, L["levels"])
        assert not L["carry"]
    assert plan["items_max"] == items_max_of(launches)
    assert plan["m_max"] == max(L["hi"] - L["lo"] for L in launches)


def cut_case(hs, sizes, chunk, G):
    rel = offsets_list(sizes)
    got = run_cut(hs, rel, chunk, G)
    check_cut(rel, chunk, G, *got)
    assert_same(got, model_cut(rel, chunk, G))
    return got


def whole_case(hs, sizes, chunk, G, t_big):
    rel = offsets_list(sizes)
    got = run_whole(hs, rel, chunk, G, t_big)
    check_whole(rel, chunk, G, t_big, *got)
    assert_same(got, model_whole(rel, chunk, G, t_big))
    return got


# ------------------------------------------------------------------ the tests
@pytest.mark.parametrize("G", [8, 16])
def test_levels_of_arbitrary_ranges(hs, G):
    rnd = random.Random(10 + G)
    cases = [[(0, 0)], [(5, 5)], [(0, 1)], [(0, G)], [(0, G + 1)], [(3, 3 + G * G), (0, 0), (1, 2)], [(0, G ** 3 + 1)], [(7, 7), (7, 7), (7, 40)]]
    for _ in range(300):                                    # ranges need not be contiguous, nor ordered
        ranges = []
        for _ in range(rnd.randint(1, 11)):
            a = rnd.randrange(50)
            ranges.append((a, a + rnd.choice(SIZES)))
        cases.append(ranges)
    for ranges in cases:
        start, ln, plan = run_levels(hs, ranges, G)
        (L,) = plan["launches"]
        check_levels(ranges, G, start, ln, L["levels"])
        ws, wl = [], []
        assert L["levels"] == model_levels(ranges, G, ws, wl)
        assert_same((start, ln, plan), (ws, wl, {"items_max": items_max_of([L]), "m_max": 0, "launches": [L]}))


@pytest.mark.parametrize("chunk", [8, 64])
@pytest.mark.parametrize("sizes", NAMED, ids=str)
def test_named_cases(hs, sizes, chunk):
    for G in (8, 16):
        cut_case(hs, sizes, chunk, G)
        whole_case(hs, sizes, chunk, G, T_BIG)


@pytest.mark.parametrize("chunk", [8, 64])
@pytest.mark.parametrize("sizes", [[3, 50, 4], [50]], ids=str)
def test_hand_over_groups(hs, sizes, chunk):
    for G in (8, 16):
        start, ln, plan = whole_case(hs, sizes, chunk, G, 20)
        big = sizes.index(50)
        touching = [L for L in plan["launches"] if L["ga"] <= big < L["gb"]]
        assert len(touching) == (7 if chunk == 8 else 1)    # cut at every multiple of the chunk it spans: 8, 16, .. 48
        assert all(ln[L["levels"][0][0] + big - L["ga"]] == 0 for L in touching)       # (the groups before it are single runs)


def test_what_the_named_cases_are_about(hs):
    # a group larger than a chunk between small ones: cut inside the group, carried into the following launches
    _, _, plan = cut_case(hs, [3, 100, 0, 2], 8, 8)
    L = plan["launches"]
    assert [(x["lo"], x["hi"]) for x in L[:3]] == [(0, 3), (3, 11), (11, 19)]
    assert [x["carry"] for x in L[:3]] == [False, False, True] and (L[1]["ga"], L[1]["gb"]) == (1, 2) == (L[2]["ga"], L[2]["gb"])
    assert (L[-1]["hi"], L[-1]["gb"]) == (105, 4)
    # the same groups as whole groups: the group of 100 alone exceeds the chunk and still gets one launch, which ends behind it
    _, _, plan = whole_case(hs, [3, 100, 0, 2], 8, 16, T_BIG)
    assert [(x["lo"], x["hi"], x["ga"], x["gb"]) for x in plan["launches"]] == [(0, 3, 0, 1), (3, 103, 1, 2), (103, 105, 2, 4)]
    assert plan["m_max"] == 100
    # trailing empty groups go to the last launch; no items at all is one launch of every group
    _, _, plan = cut_case(hs, [5, 0, 0], 8, 8)
    assert [(x["ga"], x["gb"]) for x in plan["launches"]] == [(0, 3)]
    _, _, plan = cut_case(hs, [0, 0, 0], 64, 8)
    assert [(x["lo"], x["hi"], x["ga"], x["gb"]) for x in plan["launches"]] == [(0, 0, 0, 3)]


def test_seeded_random_sweep(hs):
    rnd = random.Random(20261017)
    for _ in range(3000):
        sizes = [rnd.choice(SIZES) for _ in range(rnd.randint(1, 11))]
        chunk, G = rnd.choice((8, 16, 64, 512)), rnd.choice((8, 16))
        cut_case(hs, sizes, chunk, G)
        whole_case(hs, sizes, chunk, G, rnd.choice((20, T_BIG)))
