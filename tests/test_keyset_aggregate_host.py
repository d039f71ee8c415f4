"""CPU-only: the lane functions of the checked signature aggregation over a registered key set (bls-bn254_amd/csrc/keyset_agg.h)
compiled for the host with -DBN_CHECK, and the plain C++ of its host side (keyset_agg_plan.h): candidate bits, row assembly, the
argument walk and the repack of failing groups against a Python model, each over launch cuts at several positions.  A test
tool; the product has no CPU path."""
import ctypes
import random

import numpy as np
import pytest

from tests import hostsim_build
from tests.helpers import b32, bitmap, launches, model_candidate, u32, u64

u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)
KA_OK, KA_OFF_DECREASE, KA_TOO_MANY, KA_IDX_RANGE, KA_IDX_ORDER = range(5)
N_KEYS = 70
EDGE = [0, 31, 32, 63, 64, 69]                   # first and last key of every 32-key word of a 70-key set


@pytest.fixture(scope="module")
def hs():
    so = hostsim_build.build("keyset_aggregate_host.cpp", "libkeysetaggregatehost.so")
    lib = ctypes.CDLL(so)
    lib.hs_ka_repack.restype = ctypes.c_size_t
    return lib


def scan(hs, key_valid, idx, sigs, mask, cuts):
    cand, ident = [], []
    for lo, hi in launches(len(idx), cuts):
        c = ctypes.create_string_buffer(hi - lo); z = ctypes.create_string_buffer(hi - lo)
        hs.hs_ka_scan(bytes(key_valid), idx.ctypes.data_as(u32p), sigs, mask, lo, hi - lo, c, z)
        cand += list(c.raw); ident += list(z.raw)
    return cand, ident


def test_candidate_bits(hs, oracle, pyref):
    from tests import synth
    P = synth.P
    G = oracle.g1_generator()
    pts = [oracle.g1_mul(G, k) for k in (1, 2, 12345, pyref.R - 1)]
    off = bytearray(pts[1]); off[63] ^= 1
    big_x = b32(P) + pts[0][32:]
    big_y = pts[0][:32] + b32(P + 1)
    ident = bytes(32) + b32(1)
    sigs = pts + [bytes(off), big_x, big_y, ident, bytes(64), b"\xff" * 64, pts[2]]
    shape = [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1]                        # what the list above is made to be
    assert [int(model_candidate(s, P)) for s in sigs] == shape
    n = len(sigs)
    idx = u32([0, 3, 5, 69, 1, 2, 4, 6, 7, 8, 68])
    rnd = random.Random(5)
    all_valid = [1] * N_KEYS
    some_valid = [1] * N_KEYS
    for k in (3, 68, 7):
        some_valid[k] = 0                                             # a valid signature on a key without the KeyValidate byte
    masks = [None, [True] * n, [False] * n, [rnd.random() < 0.5 for _ in range(n)]]
    for cuts in ([], [3], [5, 6], [8], list(range(1, n))):
        for key_valid in (all_valid, some_valid, [0] * N_KEYS):
            for mask in masks:
                want = [int(shape[s] and key_valid[idx[s]] and (mask is None or mask[s])) for s in range(n)]
                cand, z = scan(hs, key_valid, idx, b"".join(sigs), None if mask is None else bitmap(mask), cuts)
                assert cand == want, (cuts, key_valid[3], mask)
                assert z == [1 - c for c in want], "a non-candidate is stored as the identity, a candidate as its point"


def rows_of(hs, idx, cand, goff, cuts):
    ng, W, rb = len(goff) - 1, (N_KEYS + 31) // 32, (N_KEYS + 7) // 8
    rows = ctypes.create_string_buffer(b"\xaa" * (ng * rb), ng * rb)   # every byte of every row must be written
    for lo, hi in launches(ng * W, cuts):
        hs.hs_ka_rows(idx.ctypes.data_as(u32p), bitmap(cand), goff.ctypes.data_as(u32p), lo, hi - lo, N_KEYS, rows)
    return [rows.raw[g * rb:(g + 1) * rb] for g in range(ng)]


def model_rows(idx, cand, goff):
    out = []
    for g in range(len(goff) - 1):
        r = bytearray((N_KEYS + 7) // 8)
        for s in range(int(goff[g]), int(goff[g + 1])):
            if cand[s]:
                r[idx[s] >> 3] |= 1 << (idx[s] & 7)
        out.append(bytes(r))
    return out


@pytest.mark.parametrize("cuts", [[], [4], [1, 2, 3], [5, 7, 11, 13], list(range(1, 18))])
def test_row_assembly(hs, cuts):
    rnd = random.Random(11)
    groups = [EDGE, [], list(range(N_KEYS)), [31], sorted(rnd.sample(range(N_KEYS), 20)), [32, 63], []]
    idx = u32([k for g in groups for k in g])
    goff = u32(np.concatenate([[0], np.cumsum([len(g) for g in groups])]))
    n = len(idx)
    for name, cand in (("ones", [True] * n), ("zeros", [False] * n), ("random", [rnd.random() < 0.6 for _ in range(n)])):
        got, want = rows_of(hs, idx, cand, goff, cuts), model_rows(idx, cand, goff)
        assert got == want, (name, cuts)
    # closed forms: all candidates -> exactly the signer set; the empty group and the group with every key
    got = rows_of(hs, idx, [True] * n, goff, cuts)
    assert got[0] == bytes([0x01, 0, 0, 0x80, 0x01, 0, 0, 0x80, 0x21])
    assert got[1] == bytes(9) and got[6] == bytes(9)
    assert got[2] == b"\xff" * 8 + b"\x3f"


def walk(hs, idx, off, n_groups, max_entries=1 << 23):
    where = (ctypes.c_uint64 * 2)()
    idx, off = u32(idx), u64(off)
    code = hs.hs_ka_walk(idx.ctypes.data_as(u32p), off.ctypes.data_as(u64p), ctypes.c_size_t(n_groups), ctypes.c_size_t(N_KEYS), ctypes.c_uint64(max_entries), where)
    return code, where[0], where[1]


def test_argument_walk(hs):
    assert walk(hs, [0, 5, 69], [0, 3], 1)[0] == KA_OK                               # a group starting at index 0, up to the last key
    assert walk(hs, [7], [0, 1], 1)[0] == KA_OK                                      # a single entry
    assert walk(hs, [9, 9, 9, 4, 8, 2], [3, 5, 5, 6], 3)[0] == KA_OK                 # non-zero first offset: the entries before it are not looked at
    assert walk(hs, [5, 4, 3, 3], [0, 1, 2, 3, 4], 4)[0] == KA_OK                    # order is per group, not across groups
    assert walk(hs, [], [0, 0, 0], 2)[0] == KA_OK
    assert walk(hs, [1, 4, 4], [0, 3], 1) == (KA_IDX_ORDER, 0, 2)                    # equal neighbours
    assert walk(hs, [1, 2, 6, 5], [0, 2, 4], 2) == (KA_IDX_ORDER, 1, 3)              # decreasing
    assert walk(hs, [1, N_KEYS], [0, 2], 1) == (KA_IDX_RANGE, 0, 1)                  # index == n_keys
    assert walk(hs, [1, 2], [0, 2, 1], 2)[:2] == (KA_OFF_DECREASE, 1)
    assert walk(hs, [1, 2, 3], [0, 3], 1, max_entries=2)[0] == KA_TOO_MANY
    assert walk(hs, [1, 2, 3], [0, 3], 1, max_entries=3)[0] == KA_OK


def test_repack_of_failing_groups(hs):
    rb = (N_KEYS + 7) // 8
    groups = [[0, 31, 32], [5], [], [1, 2, 64, 69], [8, 9]]
    lead = 2                                                            # the call's offsets start at 2
    idx = u32([99, 99] + [k for g in groups for k in g])
    off = u64(lead + np.concatenate([[0], np.cumsum([len(g) for g in groups])]))
    cand = [[1, 0, 1], [1], [], [0, 1, 1, 1], [0, 0]]
    rows = bytearray(rb * len(groups))
    for g, (ks, cs) in enumerate(zip(groups, cand)):
        for k, c in zip(ks, cs):
            if c:
                rows[g * rb + (k >> 3)] |= 1 << (k & 7)
    for fail in ([0, 3], [3], [1, 2, 4], [0, 1, 2, 3, 4], []):
        n = len(idx)
        io, po, oo = (ctypes.c_uint32 * n)(), (ctypes.c_uint64 * n)(), (ctypes.c_uint64 * (len(fail) + 1))()
        f = u64(fail)
        cnt = hs.hs_ka_repack(f.ctypes.data_as(u64p), ctypes.c_size_t(len(fail)), idx.ctypes.data_as(u32p), off.ctypes.data_as(u64p), bytes(rows),
                              ctypes.c_size_t(rb), io, po, oo)
        want_idx, want_pos, want_off = [], [], [0]
        for g in fail:
            for j, (k, c) in enumerate(zip(groups[g], cand[g])):
                if c:
                    want_idx.append(k); want_pos.append(int(off[g]) + j)
            want_off.append(len(want_idx))
        assert cnt == len(want_idx) and list(io)[:cnt] == want_idx and list(po)[:cnt] == want_pos and list(oo) == want_off, fail
        assert all(int(idx[p]) == k for p, k in zip(want_pos, want_idx))
