"""CPU-only: the lane functions of the checked merge of partial aggregates over a registered key set
(bls-bn254_amd/csrc/keyset_merge.h) compiled for the host with -DBN_CHECK, a wave run as 64 lane states in lockstep with the
votes formed by the harness, and the plain C++ of its host side (keyset_merge_plan.h): the signature test, the greedy selection
against a sequential Python model at every row width at which the code takes another path, the argument walk and the repack of
failing groups.  A test tool; the product has no CPU path."""
import ctypes
import random

import numpy as np
import pytest

from tests import hostsim_build
from tests.helpers import b32, bitmap, model_candidate, row_of, u32, u64

u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)
KM_OK, KM_OFF_DECREASE, KM_TOO_MANY, KM_ROWS_TOO_LARGE, KM_ROW_PAD = range(5)
USED, CAND = 1, 2
# n_keys -> (words, row bytes): one word; three words and 9-byte rows; 64 words, the last width with the union in a register
# (255-byte rows); 65 and 130 words, the strided form with one lane / several lanes owning two or three words
WIDTHS = {13: (1, 2), 70: (3, 9), 2035: (64, 255), 2050: (65, 257), 4133: (130, 517)}


@pytest.fixture(scope="module")
def hs():
    so = hostsim_build.build("keyset_merge_host.cpp", "libkeysetmergehost.so")
    lib = ctypes.CDLL(so)
    lib.hs_km_repack.restype = ctypes.c_size_t
    return lib


def model_select(groups, sig_ok, mask, valid, n):
    """sequential: per contribution its byte, per group the union.  groups: lists of key sets; valid: the set of valid keys"""
    flags, unions, s = [], [], 0
    for g in groups:
        union = set()
        for keys in g:
            cand = bool(sig_ok[s]) and len(keys) > 0 and keys <= valid
            used = cand and (mask is None or mask[s]) and not (keys & union)
            if used:
                union |= keys
            flags.append((CAND if cand else 0) | (USED if used else 0))
            s += 1
        unions.append(row_of(union, n))
    return flags, unions


def run_select(hs, groups, sig_ok, mask, valid, n, cuts):
    W, rb = (n + 31) // 32, (n + 7) // 8
    rows = b"".join(row_of(k, n) for g in groups for k in g)
    goff = u32(np.concatenate([[0], np.cumsum([len(g) for g in groups])]))
    N, ng = int(goff[-1]), len(groups)
    vw = u32([sum(1 << b for b in range(32) if 32 * w + b in valid) for w in range(W)])
    flags = ctypes.create_string_buffer(b"\xee" * max(N, 1), max(N, 1))
    urows = ctypes.create_string_buffer(b"\xaa" * (ng * rb), ng * rb)       # every byte of every merged row must be written
    edges = [0] + [c for c in cuts if 0 < c < ng] + [ng]
    for lo, hi in zip(edges, edges[1:]):
        hs.hs_km_select(rows + b"\0", bytes(sig_ok) + b"\0", None if mask is None else bitmap(mask), goff.ctypes.data_as(u32p), vw.ctypes.data_as(u32p), n, lo, hi - lo,
                        flags, urows)
    return list(flags.raw[:N]), [urows.raw[g * rb:(g + 1) * rb] for g in range(ng)]


def edge_keys(n):
    """the first and last key of the words at which lanes change hands"""
    W = (n + 31) // 32
    ws = sorted({w for w in (0, 1, 62, 63, 64, 65, 127, 128, W - 1) if w < W})
    return sorted({k for w in ws for k in (32 * w, min(32 * w + 31, n - 1))})


@pytest.mark.parametrize("n", sorted(WIDTHS))
def test_widths(n):
    assert ((n + 31) // 32, (n + 7) // 8) == WIDTHS[n] and all(rb % 4 for _, rb in WIDTHS.values())


@pytest.mark.parametrize("n", sorted(WIDTHS))
def test_selection_against_the_model(hs, n):
    rnd = random.Random(900 + n)
    edge = edge_keys(n)
    invalid = {edge[-1], edge[len(edge) // 2]} if n > 13 else {n - 1}
    valid = set(range(n)) - invalid
    ok_keys = sorted(valid)

    def some(k):
        return set(rnd.sample(ok_keys, min(k, len(ok_keys))))

    a = some(5)
    b = set([k for k in ok_keys if k not in a][:3])
    groups = [
        [{k} for k in edge if k in valid],                                 # disjoint single keys at every lane hand-over: all used
        [a, set(a), b, set()],                                              # a duplicate, a row beside them, an empty row
        [],                                                                 # no contribution
        [some(3) | {min(invalid)}, {max(invalid)}, some(2)],                # rows that select an invalid key: no candidates
        [set(valid), some(1)],                                              # every valid key, then anything overlaps
        [{ok_keys[0], ok_keys[-1]}, {ok_keys[-1]}, {ok_keys[1]}, {ok_keys[0]}, {ok_keys[2], ok_keys[-2]}],   # overlaps in the first and the last word
        [set(range(n))],                                                    # every key, the invalid ones too
    ] + [[some(rnd.randrange(0, 6)) for _ in range(rnd.randrange(1, 7))] for _ in range(6)]
    N = sum(len(g) for g in groups)
    sig_sets = [[1] * N, [rnd.random() < 0.8 for _ in range(N)]]
    masks = [None, [True] * N, [False] * N, [rnd.random() < 0.6 for _ in range(N)]]
    for cuts in ([], [1, 2, 5], list(range(1, len(groups)))):
        for sig_ok in sig_sets:
            for mask in masks:
                want = model_select(groups, sig_ok, mask, valid, n)
                got = run_select(hs, groups, sig_ok, mask, valid, n, cuts)
                assert got == want, (n, cuts, mask is None)
    # closed forms, all signatures good and no mask
    flags, unions = run_select(hs, groups, [1] * N, None, valid, n, [])
    n0 = len(groups[0])
    assert flags[:n0] == [CAND | USED] * n0 and unions[0] == row_of([k for k in edge if k in valid], n)
    assert flags[n0:n0 + 4] == [CAND | USED, CAND, CAND | USED, 0] and unions[2] == bytes((n + 7) // 8)
    assert flags[n0 + 4:n0 + 7] == [0, 0, CAND | USED]
    assert unions[4] == row_of(valid, n) and flags[n0 + 7:n0 + 9] == [CAND | USED, CAND]
    assert flags[n0 + 9:n0 + 14] == [CAND | USED, CAND, CAND | USED, CAND, CAND | USED]
    assert flags[n0 + 14] == 0 and unions[6] == bytes((n + 7) // 8)


@pytest.mark.parametrize("n", sorted(WIDTHS))
def test_admissible_once_an_earlier_one_is_masked_out(hs, n):
    """[A, B, C] with B overlapping A only and C overlapping B only: without a mask A and C are used; with A masked out B is
    used and C is not -- the fallback's second selection"""
    last = n - 1
    A, B, C = {0, last}, {last, 1} if n > 2 else {last}, {1, 2}
    valid = set(range(n))
    flags, unions = run_select(hs, [[A, B, C]], [1, 1, 1], None, valid, n, [])
    assert flags == [CAND | USED, CAND, CAND | USED] and unions == [row_of(A | C, n)]
    flags, unions = run_select(hs, [[A, B, C]], [1, 1, 1], [False, True, True], valid, n, [])
    assert flags == [CAND, CAND | USED, CAND] and unions == [row_of(B, n)]
    flags, unions = run_select(hs, [[A, B, C]], [0, 1, 1], None, valid, n, [])            # the same through the signature byte
    assert flags == [0, CAND | USED, CAND] and unions == [row_of(B, n)]


def test_signature_bytes_and_dropped_points(hs, oracle, pyref):
    from tests import synth
    P = synth.P
    G = oracle.g1_generator()
    pts = [oracle.g1_mul(G, k) for k in (1, 2, 12345, pyref.R - 1)]
    off = bytearray(pts[1]); off[63] ^= 1
    sigs = pts + [bytes(off), b32(P) + pts[0][32:], pts[0][:32] + b32(P + 1), bytes(32) + b32(1), bytes(64), b"\xff" * 64, pts[2]]
    shape = [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1]
    assert [int(model_candidate(s, P)) for s in sigs] == shape
    n = len(sigs)
    for cuts in ([], [3], [5, 6], list(range(1, n))):
        edges = [0] + cuts + [n]
        ok, ident = [], []
        for lo, hi in zip(edges, edges[1:]):
            o = ctypes.create_string_buffer(hi - lo); z = ctypes.create_string_buffer(hi - lo)
            hs.hs_km_sig(b"".join(sigs), lo, hi - lo, o, z)
            ok += list(o.raw); ident += list(z.raw)
        assert ok == shape and ident == [1 - c for c in shape], cuts
    flags = bytes([0, CAND, CAND | USED, 0, CAND | USED, CAND])
    z = ctypes.create_string_buffer(4)
    hs.hs_km_points(flags, 1, 4, z)
    assert list(z.raw) == [1, 0, 1, 0], "an unused contribution's point becomes the identity, a used one's is left alone"


def walk(hs, rows, off, n_groups, n_keys, max_con=1 << 23, max_bytes=1 << 30):
    where = (ctypes.c_uint64 * 2)()
    off = u64(off)
    code = hs.hs_km_walk(rows, off.ctypes.data_as(u64p), ctypes.c_size_t(n_groups), ctypes.c_size_t(n_keys), ctypes.c_uint64(max_con), ctypes.c_uint64(max_bytes), where)
    return code, where[0], where[1]


def test_argument_walk(hs):
    n = 13                                                                  # two bytes per row, three padding bits
    good = [row_of(k, n) for k in ({0}, {12}, set(), set(range(13)))]
    pad = bytes([0, 0x20])                                                  # bit 13
    assert walk(hs, b"".join(good), [0, 2, 2, 4], 3, n)[0] == KM_OK
    assert walk(hs, pad + b"".join(good), [1, 3, 5], 2, n)[0] == KM_OK      # non-zero first offset: the row before it is not looked at
    assert walk(hs, b"".join(good) + pad, [0, 2, 4], 2, n)[0] == KM_OK      # ... nor the row behind the last offset
    assert walk(hs, b"", [0, 0, 0], 2, n)[0] == KM_OK
    assert walk(hs, good[0] + good[1] + pad + good[3], [0, 1, 4], 2, n) == (KM_ROW_PAD, 1, 2)
    assert walk(hs, good[0] + bytes([0, 0x80]), [0, 2], 1, n) == (KM_ROW_PAD, 0, 1)
    assert walk(hs, b"\xff\xff", [0, 1], 1, 16)[0] == KM_OK                 # n_keys a multiple of 8: no padding bits
    assert walk(hs, b"".join(good), [0, 3, 2], 2, n)[:2] == (KM_OFF_DECREASE, 1)
    assert walk(hs, b"".join(good), [0, 4], 1, n, max_con=3)[0] == KM_TOO_MANY
    assert walk(hs, b"".join(good), [0, 4], 1, n, max_con=4)[0] == KM_OK
    assert walk(hs, b"".join(good), [0, 4], 1, n, max_bytes=7)[0] == KM_ROWS_TOO_LARGE
    assert walk(hs, b"".join(good), [0, 4], 1, n, max_bytes=8)[0] == KM_OK
    assert walk(hs, b"".join(good), [0, 3, 2], 2, n, max_con=0)[0] == KM_OFF_DECREASE     # the offsets come first


def test_repack_of_failing_groups(hs):
    n = 70
    rb = (n + 7) // 8
    rnd = random.Random(7)
    sizes = [3, 1, 0, 4, 2]
    lead = 2                                                                # the call's offsets start at 2
    N = lead + sum(sizes)
    rows = [bytes(rnd.randrange(256) for _ in range(rb)) for _ in range(N)]
    sigs = [bytes(rnd.randrange(256) for _ in range(64)) for _ in range(N)]
    off = u64(lead + np.concatenate([[0], np.cumsum(sizes)]))
    cand = [1, 0, 1, 1, 0, 1, 1, 1, 0, 0]                                   # by contribution of the call, from its first one
    for fail in ([0, 3], [3], [1, 2, 4], [0, 1, 2, 3, 4], []):
        po, oo = (ctypes.c_uint64 * N)(), (ctypes.c_uint64 * (len(fail) + 1))()
        ro, so = ctypes.create_string_buffer(N * rb), ctypes.create_string_buffer(N * 64)
        f = u64(fail)
        cnt = hs.hs_km_repack(f.ctypes.data_as(u64p), ctypes.c_size_t(len(fail)), b"".join(rows), b"".join(sigs), off.ctypes.data_as(u64p), bitmap(cand),
                              ctypes.c_size_t(rb), po, oo, ro, so)
        want_pos, want_off = [], [0]
        for g in fail:
            want_pos += [s for s in range(int(off[g]), int(off[g + 1])) if cand[s - lead]]
            want_off.append(len(want_pos))
        assert cnt == len(want_pos) and list(po)[:cnt] == want_pos and list(oo) == want_off, fail
        assert ro.raw[:cnt * rb] == b"".join(rows[p] for p in want_pos) and so.raw[:cnt * 64] == b"".join(sigs[p] for p in want_pos)
