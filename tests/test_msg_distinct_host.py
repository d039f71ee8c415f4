"""CPU-only: msg_distinct.h compiled for the host with -DBN_CHECK (tests/hostsim/msg_distinct_host.cpp; the common hostsim flags)
and run lane by lane against the model of tests/msg_distinct_support.py: the keys byte for byte, every slot of the table and every
dup byte.  Table sizes: the minimal legal one, and tiny ones (mask 1 and 3 with more keys than slots) where long probe chains, the
wrap-around and the fail-closed bound all run; a second build whose slot hash sends every key to slot 0; equal points in
different groups; one value in several limb patterns; the homogeneous form with z != 1 on both sides; every insertion order of a
4-pair group with a triple repeat.  The same main file, built as a program of its own with the address and undefined-behaviour
sanitizers, is run once as a child process.  A test tool; the product has no CPU path."""
import ctypes
import itertools
import random
import subprocess

import numpy as np
import pytest

from tests import hostsim_build
from tests import msg_distinct_support as D

P = D.P


def bind(path):
    hs = ctypes.CDLL(path)
    hs.hs_md_slots.restype = ctypes.c_uint32
    hs.hs_md_slot_hash.restype = ctypes.c_uint32
    hs.hs_md_group_of.restype = ctypes.c_uint32
    return hs


@pytest.fixture(scope="module")
def hs():
    return bind(hostsim_build.build("msg_distinct_host.cpp", "libmsgdistinct.so"))


@pytest.fixture(scope="module")
def hs_zero():
    return bind(hostsim_build.build("msg_distinct_host.cpp", "libmsgdistinct_zero.so", extra=["-DMD_SLOT_HASH_ZERO"]))


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def limbs(hs, v, pattern=0):
    """the 9 limbs of the value v as a workspace may hold it: 0 canonical, 1 with p added limb by limb, 2 with one unit of limb
    1 moved down into limb 0 (limb 1 may go negative)"""
    out = np.zeros(9, dtype=np.int32)
    assert hs.hs_md_fp_limbs(v.to_bytes(32, "big"), ptr(out)) == 1
    if pattern == 1:
        p = np.zeros(9, dtype=np.int32)
        hs.hs_md_p_limbs(ptr(p))
        out = out + p
    elif pattern == 2:
        out[0] += 1 << 29
        out[1] -= 1
    return out


def workspace(hs, coords, patterns):
    """coords: per pair a tuple of 2 (affine) or 3 (homogeneous) values; limb-major, stride = the number of pairs"""
    n, rows = len(coords), 9 * len(coords[0])
    ws = np.zeros((rows, n), dtype=np.int32)
    for i, c in enumerate(coords):
        for j, v in enumerate(c):
            ws[9 * j:9 * j + 9, i] = limbs(hs, v % P, patterns[i][j])
    return np.ascontiguousarray(ws)


def keys_of(hs, ws, form):
    n = ws.shape[1]
    key = np.zeros((18, n), dtype=np.int32)
    hs.hs_md_keys(ptr(ws), ctypes.c_size_t(n), n, form, ptr(key))
    return key


def key_points(hs, key):
    n = key.shape[1]
    out = []
    for i in range(n):
        b = ctypes.create_string_buffer(64)
        hs.hs_md_key_bytes(ptr(key), n, i, b)
        out.append((int.from_bytes(b.raw[:32], "big"), int.from_bytes(b.raw[32:], "big")))
    return out


def run_table(hs, key, goff, order, M, seed):
    n, G = key.shape[1], len(goff) - 1
    go, od = np.array(goff, dtype=np.uint32), np.array(order, dtype=np.uint32)
    slots, dup = np.full(M, 0x12345678, dtype=np.uint32), np.full(max(G, 1), 0xcc, dtype=np.uint8)
    hs.hs_md_insert_all(n, ptr(go), G, ptr(key), ptr(od), ptr(slots), M - 1, seed, ptr(dup))
    return slots.tolist(), dup[:G].tolist()


def check_against_model(hs, key, points, goff, order, M, seed, zero=False):
    n = key.shape[1]
    start = (lambda g, i: 0) if zero else (lambda g, i: hs.hs_md_slot_hash(g, ptr(key), n, i, seed))
    got = run_table(hs, key, goff, order, M, seed)
    want = D.table_model(points, goff, order, M, start)
    assert got == (want[0], want[1]), (goff, order, M)
    return got[1]


def random_case(hs, rnd, n, goff, distinct):
    """n affine pairs over `distinct` points, in random limb patterns"""
    pool = [(rnd.randrange(P), rnd.randrange(P)) for _ in range(distinct)]
    pts = [pool[rnd.randrange(distinct)] for _ in range(n)]
    ws = workspace(hs, pts, [(rnd.randrange(3), rnd.randrange(3)) for _ in range(n)])
    return pts, keys_of(hs, ws, D.AFFINE)


def test_slots_and_groups(hs):
    for n in (0, 1, 2, 3, 4, 5, 64, 65, 130, 1 << 23):
        assert hs.hs_md_slots(n) == D.slots_for(n)
    goff = np.array([3, 3, 4, 6, 6, 6, 9, 20], dtype=np.uint32)
    for i in range(3, 20):
        assert hs.hs_md_group_of(ptr(goff), 7, i) == D.group_of(goff.tolist(), i), i


def test_keys_are_canonical_values(hs):
    rnd = random.Random(11)
    vals = [0, 1, P - 1, P - 2, (1 << 29) - 1, 1 << 29, 1 << 232] + [rnd.randrange(P) for _ in range(9)]
    pts = [(v, (v * 7 + 3) % P) for v in vals]
    keys = [keys_of(hs, workspace(hs, pts, [(a, b)] * len(pts)), D.AFFINE) for a in range(3) for b in range(3)]
    for k in keys:
        assert key_points(hs, k) == pts
        assert (k == keys[0]).all()                       # one value, several limb patterns: ONE key


def test_homogeneous_form_normalises(hs):
    rnd = random.Random(12)
    pts = [(rnd.randrange(P), rnd.randrange(P)) for _ in range(6)]
    pts[3] = pts[1]                                        # the same point under two different z, neither of them 1
    zs = [rnd.randrange(2, P) for _ in pts]
    hom = [(x * z % P, y * z % P, z) for (x, y), z in zip(pts, zs)]
    key = keys_of(hs, workspace(hs, hom, [(i % 3, (i + 1) % 3, (i + 2) % 3) for i in range(6)]), D.HOMOGENEOUS)
    assert key_points(hs, key) == pts
    assert (key[:, 3] == key[:, 1]).all()
    aff = keys_of(hs, workspace(hs, pts, [(0, 0)] * 6), D.AFFINE)
    assert (key == aff).all()
    goff = [0, 6]
    assert check_against_model(hs, key, pts, goff, range(6), 16, 77) == [1]
    # z = 0: the identity, keyed as its encoding (0, 1)
    ident = keys_of(hs, workspace(hs, [(5, 9, 0), (0, 1, 1)], [(0, 0, 0)] * 2), D.HOMOGENEOUS)
    assert key_points(hs, ident) == [(0, 1), (0, 1)]


@pytest.mark.parametrize("seed", [0, 1, 0xffffffff])
def test_minimal_table_against_model(hs, hs_zero, seed):
    rnd = random.Random(20 + (seed & 7))
    goff = [3, 3, 4, 6, 9, 9, 18, 23, 23]
    n = 25                                                 # three pairs in front of the first group, two behind the last
    pts, key = random_case(hs, rnd, n, goff, 12)
    pts[0] = pts[3]; pts[24] = pts[22]                     # equal to pairs inside groups, themselves in no group
    pts[4] = pts[5]                                        # a repeat for certain
    key = keys_of(hs, workspace(hs, pts, [(i % 3, (i // 3) % 3) for i in range(n)]), D.AFFINE)
    want = D.dup_of(pts, goff)
    assert want[2] and not want[0] and not want[1] and not want[4] and not want[7]
    for order in (list(range(n)), list(range(n - 1, -1, -1)), rnd.sample(range(n), n)):
        M = D.slots_for(n)
        assert check_against_model(hs, key, pts, goff, order, M, seed) == [int(b) for b in want]
        assert check_against_model(hs_zero, key, pts, goff, order, M, seed, zero=True) == [int(b) for b in want]


def test_equal_points_in_different_groups(hs, hs_zero):
    rnd = random.Random(30)
    a, b = (rnd.randrange(P), rnd.randrange(P)), (rnd.randrange(P), rnd.randrange(P))
    pts = [a, b, a, b, a, a]                               # groups {a, b}, {a, b}, {a, a}
    goff = [0, 2, 4, 6]
    key = keys_of(hs, workspace(hs, pts, [(i % 3, 0) for i in range(6)]), D.AFFINE)
    for lib, zero in ((hs, False), (hs_zero, True)):
        for order in itertools.permutations(range(6)):
            if order[0] > 1:                               # a sixth of the 720 orders is enough for the slow build
                continue
            assert check_against_model(lib, key, pts, goff, list(order), 16, 5, zero=zero) == [0, 0, 1]


@pytest.mark.parametrize("M", [2, 4])
def test_tiny_tables_fail_closed(hs, hs_zero, M):
    """more keys than slots: the probe chain wraps around the table and ends after M slots, marking its group"""
    rnd = random.Random(40 + M)
    goff = [0, 1, 3, 3, 9]
    pts, key = random_case(hs, rnd, 9, goff, 50)
    assert len(set(pts)) == 9                              # no real repeat: whatever is marked is the bound's doing
    for lib, zero in ((hs, False), (hs_zero, True)):
        for order in (list(range(9)), list(range(8, -1, -1)), rnd.sample(range(9), 9)):
            dup = check_against_model(lib, key, pts, goff, order, M, 3, zero=zero)
            assert dup[2] == 0                             # an empty group is never marked
            assert sum(1 for g in (0, 1, 3) if dup[g]) >= 1 and dup[3] == 1      # nine keys, M slots: the large group cannot fit
    # with a real repeat the mark survives whichever way it comes about
    pts[4] = pts[3]
    key = keys_of(hs, workspace(hs, pts, [(0, 0)] * 9), D.AFFINE)
    assert check_against_model(hs, key, pts, goff, list(range(9)), M, 3)[3] == 1


def test_every_order_of_a_triple_repeat(hs, hs_zero):
    rnd = random.Random(50)
    a, b = (rnd.randrange(P), rnd.randrange(P)), (rnd.randrange(P), rnd.randrange(P))
    pts = [a, b, a, a]
    key = keys_of(hs, workspace(hs, pts, [(0, 1), (2, 0), (1, 2), (2, 2)]), D.AFFINE)
    for lib, zero in ((hs, False), (hs_zero, True)):
        for order in itertools.permutations(range(4)):
            assert check_against_model(lib, key, pts, [0, 4], list(order), D.slots_for(4), 9, zero=zero) == [1]
    key2 = keys_of(hs, workspace(hs, [a, b, (a[0], b[1]), (b[0], a[1])], [(0, 0)] * 4), D.AFFINE)      # equal x or equal y alone is no repeat
    for order in itertools.permutations(range(4)):
        assert run_table(hs_zero, key2, [0, 4], list(order), 8, 9)[1] == [0]


def test_sanitized_program_runs_clean(tmp_path_factory):
    """the lane functions alone, as an ordinary program with its own main: nothing is loaded into this process.  The common
    recipe plus the sanitizers; -fno-sanitize=shift because the field code shifts signed limbs left by design (fp29.h fp_lc)"""
    exe = tmp_path_factory.mktemp("msg_distinct_host") / "msg_distinct_host"
    prog = hostsim_build.build("msg_distinct_host.cpp", exe, shared=False, extra=hostsim_build.SANITIZED + ["-fno-sanitize=shift"])
    out = subprocess.run([prog], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stdout[-1000:], out.stderr[-3000:])
    assert "msg_distinct_host ok" in out.stdout
