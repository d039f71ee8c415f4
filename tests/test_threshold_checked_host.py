"""CPU-only: the lane functions of the checked threshold combine (bls-bn254_amd/csrc/threshold_checked.h) compiled for the host
with -DBN_CHECK: candidate bits, repeated ids, ranks, used bits, short marks and compacted slots against a Python model, over
ragged groups with an empty group, a group cut by a launch boundary, all-zero and all-one bitmaps and t_g == n_g.  A test tool;
the product has no CPU path."""
import ctypes
import random

import numpy as np
import pytest

from tests import hostsim_build
from tests.helpers import b32, bitmap, launches, offsets_u32

u32p = ctypes.POINTER(ctypes.c_uint32)
MARK_SCALAR, MARK_POINT, MARK_SHORT = 1, 2, 4
SIZES_N = [3, 0, 7, 5, 1, 6, 4, 9]
SIZES_T = [2, 2, 7, 3, 0, 4, 5, 1]          # t == n (group 2), t == 0 (group 4), t > n (group 6), an empty group (1)


@pytest.fixture(scope="module")
def hs():
    so = hostsim_build.build("threshold_checked_host.cpp", "libthresholdcheckedhost.so")
    return ctypes.CDLL(so)


def scan(hs, ids, sigs, goff, cuts):
    n = int(goff[-1])
    cand, rep = [], []
    for lo, hi in launches(n, cuts):
        c = ctypes.create_string_buffer(hi - lo); r = ctypes.create_string_buffer(hi - lo)
        hs.hs_tc_scan(ids, sigs, goff.ctypes.data_as(u32p), len(goff) - 1, lo, hi - lo, c, r)
        cand += list(c.raw); rep += list(r.raw)
    return cand, rep


def select(hs, bits_a, bits_b, goff, coff, marks, ids, sigs, cuts):
    n, t = int(goff[-1]), int(coff[-1])
    mk = np.array(marks, dtype=np.uint32)
    c_ids = ctypes.create_string_buffer(32 * max(t, 1)); c_sigs = ctypes.create_string_buffer(64 * max(t, 1))
    rank, used = [], []
    for lo, hi in launches(n, cuts):
        r = (ctypes.c_uint32 * (hi - lo))(); u = ctypes.create_string_buffer(hi - lo)
        hs.hs_tc_select(bits_a, bits_b, goff.ctypes.data_as(u32p), coff.ctypes.data_as(u32p), len(goff) - 1, mk.ctypes.data_as(u32p), lo, hi - lo,
                        ids, sigs, c_ids, c_sigs, r, u)
        rank += list(r); used += list(u.raw)
    return rank, used, list(mk), c_ids.raw[:32 * t], c_sigs.raw[:64 * t]


def model(bits, goff, coff, marks, ids, sigs):
    """ranks, used bits, marks and the compacted arrays by the rule of the header"""
    n, t_all = int(goff[-1]), int(coff[-1])
    rank, used, mk = [0] * n, [0] * n, list(marks)
    c_ids, c_sigs = bytearray(32 * t_all), bytearray(64 * t_all)
    for g in range(len(goff) - 1):
        a, b, t = int(goff[g]), int(goff[g + 1]), int(coff[g + 1] - coff[g])
        live = [s for s in range(a, b) if bits[s]]
        for s in range(a, b):
            rank[s] = sum(1 for j in live if j < s)
        short = t == 0 or len(live) < t
        if short and b > a:                                           # (an empty group has no lane: the per-group kernel marks it)
            mk[g] |= MARK_SHORT
        if short or (marks[g] & (MARK_SCALAR | MARK_POINT)):
            continue
        for k, s in enumerate(live[:t]):
            used[s] = 1
            c_ids[32 * (int(coff[g]) + k):32 * (int(coff[g]) + k + 1)] = ids[32 * s:32 * s + 32]
            c_sigs[64 * (int(coff[g]) + k):64 * (int(coff[g]) + k + 1)] = sigs[64 * s:64 * s + 64]
    return rank, used, mk, bytes(c_ids), bytes(c_sigs)


def test_candidate_bits(hs, oracle, pyref):
    from tests import synth
    P = synth.P
    G = oracle.g1_generator()
    pts = [oracle.g1_mul(G, k) for k in (1, 2, 12345, pyref.R - 1)]
    off = bytearray(pts[1]); off[63] ^= 1
    big_x = b32(P) + pts[0][32:]
    big_y = pts[0][:32] + b32(P + 1)
    ident = bytes(32) + b32(1)
    sigs = pts + [bytes(off), big_x, big_y, ident, bytes(64), b"\xff" * 64, bytes(32) + b"\xff" * 32]
    want = [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]                          # (x == 0 reads as the identity whatever y holds)
    n = len(sigs)
    goff = offsets_u32([4, 0, n - 4])
    ids = b"".join(b32(i + 1) for i in range(n))
    for cuts in ([], [3], [5, 6]):
        cand, rep = scan(hs, ids, b"".join(sigs), goff, cuts)
        assert cand == want and rep == [0] * n, cuts


def test_repeat_detection(hs, pyref):
    R = pyref.R
    sizes = [4, 0, 6, 3, 2]
    goff = offsets_u32(sizes)
    id_sets = [[1, 2, 3, 1], [], [9, 8, 9, 7, 9, 8], [7, 6, 7], [R + 5, R + 5]]
    id_sets[3][1] = 1                                                 # the same id as group 0's: other groups are never looked at
    ids = b"".join(b32(x) for s in id_sets for x in s)
    low = bytearray(b32(7)); low[0] = 1                                # differs from 7 in its FIRST byte only
    ids = ids[:32 * 12] + bytes(low) + ids[32 * 13:]
    want = [0, 0, 0, 1] + [0, 0, 1, 0, 1, 1] + [0, 0, 0] + [0, 1]
    sigs = bytes(64 * len(want))
    for cuts in ([], [5], [1, 6, 9, 14]):                             # group 2 (shares 4 .. 10) cut by a launch boundary
        cand, rep = scan(hs, ids, sigs, goff, cuts)
        assert rep == want and cand == [0] * len(want), cuts


@pytest.mark.parametrize("cuts", [[], [5], [8, 16, 24], list(range(1, 35))])
def test_ranks_and_compacted_slots(hs, cuts):
    rnd = random.Random(7)
    goff, coff = offsets_u32(SIZES_N), offsets_u32(SIZES_T)
    n = int(goff[-1])
    ids = rnd.randbytes(32 * n); sigs = rnd.randbytes(64 * n)
    patterns = {"random": [rnd.random() < 0.7 for _ in range(n)], "zeros": [False] * n, "ones": [True] * n}
    second = [rnd.random() < 0.6 for _ in range(n)]
    marks = [0, 0, 0, MARK_SCALAR, 0, MARK_POINT, 0, 0]
    for name, bits in patterns.items():
        for b_bits, mk in ((None, [0] * 8), (second, [0] * 8), (None, marks)):
            eff = bits if b_bits is None else [x and y for x, y in zip(bits, b_bits)]
            got = select(hs, bitmap(bits), None if b_bits is None else bitmap(b_bits), goff, coff, mk, ids, sigs, cuts)
            want = model(eff, goff, coff, mk, ids, sigs)
            for k, what in enumerate(("rank", "used", "marks", "compacted ids", "compacted signatures")):
                assert got[k] == want[k], (name, b_bits is not None, mk, what)
    # all ones and no marks: the first t_g shares of every group that is large enough, t_g == n_g included
    rank, used, mk, c_ids, c_sigs = select(hs, bitmap([True] * n), None, goff, coff, [0] * 8, ids, sigs, cuts)
    for g, (ng, t) in enumerate(zip(SIZES_N, SIZES_T)):
        a = int(goff[g])
        ok = 0 < t <= ng
        assert used[a:a + ng] == ([1] * t + [0] * (ng - t) if ok else [0] * ng), g
        assert bool(mk[g] & MARK_SHORT) == (not ok and ng > 0), g
        if ok:
            assert c_ids[32 * int(coff[g]):32 * int(coff[g + 1])] == ids[32 * a:32 * (a + t)], g
        else:
            assert c_sigs[64 * int(coff[g]):64 * int(coff[g + 1])] == bytes(64 * t), g    # untouched: what the host zeroed
