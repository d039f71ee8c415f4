"""CPU-only: the lane functions of the key-share check (bls-bn254_amd/csrc/threshold_keycheck.h) compiled for the host with
-DBN_CHECK, so every field operation asserts the lazy-limb interval discipline: the table of the generator's multiples built row
by row, its fixed-base sum against the oracle's sk_to_pk, the equality on both representatives of a point and on the identity,
and the whole check over small ragged groups against a Python Horner.  A test tool; the product has no CPU path."""
import ctypes
import random

import numpy as np
import pytest

from tests import hostsim_build
from tests.helpers import b32, bits_of, IDENT2, offsets_u32, poly_eval

u32p = ctypes.POINTER(ctypes.c_uint32)
i32p = ctypes.POINTER(ctypes.c_int32)


@pytest.fixture(scope="module")
def hs():
    lib = ctypes.CDLL(hostsim_build.build("threshold_keycheck_host.cpp", "libthresholdkeycheckhost.so"))
    lib.hs_kc_table_limbs.restype = ctypes.c_size_t
    return lib


@pytest.fixture(scope="module")
def table(hs):
    """the table, built ONCE as the kernel's lanes build it (one call per window), shared by every test of the module"""
    tab = np.zeros(hs.hs_kc_table_limbs(), dtype=np.int32)
    assert tab.ctypes.data % 8 == 0
    hs.hs_kc_table(tab.ctypes.data_as(i32p))
    tab.setflags(write=False)
    return tab


def fixed_base(hs, table, k):
    out = ctypes.create_string_buffer(128)
    ok = hs.hs_kc_fixed_base(table.ctypes.data_as(i32p), b32(k), out)
    return out.raw, ok


def test_table_shape_and_identity_entries(hs, table):
    bits, windows = hs.hs_kc_window_bits(), hs.hs_kc_windows()
    assert bits * windows == 256 and table.size == windows * (1 << bits) * 54
    rows = table.reshape(windows, 1 << bits, 54)
    for w in range(windows):                                         # entry 0 of every row: (0 : 1 : 0), Y in Montgomery form
        assert not rows[w, 0, :18].any() and not rows[w, 0, 36:].any() and rows[w, 0, 18:27].any(), w
    assert (rows >= 0).all() and (rows < (1 << 29)).all()            # canonical limbs


def test_fixed_base_sum_matches_sk_to_pk(hs, table, oracle, pyref):
    R = pyref.R
    every_low_nibble = int("2" + "f" * 63, 16)
    assert every_low_nibble < R
    rnd = random.Random(21)
    ks = [0, 1, 15, 16, 1 << 252, R - 1, every_low_nibble] + [rnd.randrange(R) for _ in range(4)]
    for k in ks:
        got, ok = fixed_base(hs, table, k)
        assert ok == 1, hex(k)
        assert got == (oracle.sk_to_pk(k) if k else IDENT2), hex(k)
    # the range flag is r's alone: zero passes, r and 2^256 - 1 do not (their sums are [k mod r] G2gen all the same)
    assert fixed_base(hs, table, R)[1] == 0 and fixed_base(hs, table, (1 << 256) - 1)[1] == 0
    assert fixed_base(hs, table, R + 5)[0] == oracle.sk_to_pk(5)


def eq(hs, table, share, commits, x, nbits, neg=False):
    zd, ai, bi = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    r = hs.hs_kc_eq(table.ctypes.data_as(i32p), b32(share), ctypes.c_int(1 if neg else 0), b"".join(commits), ctypes.c_uint32(len(commits)), b32(x),
                    ctypes.c_int(nbits), ctypes.byref(zd), ctypes.byref(ai), ctypes.byref(bi))
    return r, zd.value, ai.value, bi.value


def test_equality(hs, table, oracle, pyref):
    R = pyref.R
    rnd = random.Random(22)
    coefs = [rnd.randrange(1, R) for _ in range(3)]
    commits = [oracle.sk_to_pk(a) for a in coefs]
    s = poly_eval(coefs, 5)
    # the same point by the table and by the Horner chain: two representatives with different Z
    assert eq(hs, table, s, commits, 5, 3) == (1, 1, 0, 0)
    assert eq(hs, table, s, commits, 5, 254) == (1, 1, 0, 0)
    assert eq(hs, table, (s + 1) % R, commits, 5, 3)[0] == 0
    # the identity against the identity: no commitments and the zero share
    assert eq(hs, table, 0, [], 5, 3) == (1, 0, 1, 1)
    # ... reached the long way round: f = a - a x at x = 1
    a = coefs[0]
    assert eq(hs, table, 0, [oracle.sk_to_pk(a), oracle.sk_to_pk(R - a)], 1, 1)[0::2] == (1, 1)
    # the identity against a point, both ways
    assert eq(hs, table, 0, commits[:1], 5, 3) == (0, 1, 1, 0)
    assert eq(hs, table, 3, [], 5, 3) == (0, 1, 0, 1)
    # P against -P
    assert eq(hs, table, s, commits, 5, 3, neg=True)[0] == 0
    assert eq(hs, table, R - s, commits, 5, 3)[0] == 0
    # a share that is not canonical is refused although it names the same point
    if s + R < 1 << 256:
        assert eq(hs, table, s + R, commits, 5, 3)[0] == 0


def check(hs, table, commit_sets, id_sets, share_sets, nbits):
    coff, goff = offsets_u32([len(s) for s in commit_sets]), offsets_u32([len(s) for s in id_sets])
    n = int(goff[-1])
    bm = ctypes.create_string_buffer((n + 7) // 8 + 1)
    st = ctypes.create_string_buffer(len(id_sets))
    hs.hs_kc_check(table.ctypes.data_as(i32p), b"".join(c for s in commit_sets for c in s), coff.ctypes.data_as(u32p), b"".join(b32(x) for s in id_sets for x in s),
                   b"".join(b32(x) for s in share_sets for x in s), goff.ctypes.data_as(u32p), len(id_sets), ctypes.c_int(nbits), bm, st)
    assert bm.raw[(n + 7) // 8:] == b"\x00"
    return bits_of(bm.raw, n), list(st.raw), bm.raw[:(n + 7) // 8]


def test_whole_check_over_ragged_groups(hs, table, oracle, pyref):
    from tests import synth
    R = pyref.R
    coefs = [3, 5, 7]
    C = [oracle.sk_to_pk(k) for k in coefs]
    off_curve = bytearray(C[1]); off_curve[127] ^= 1
    # the groups of test_g2_marks_and_the_empty_polynomial, with an honest share for every id
    commit_sets = [C[:2], [], [C[0], bytes(off_curve)], [synth.NON_SUBGROUP_PK], C[:2], [b"\xff" * 128, C[2]], [C[2]], [IDENT2, C[0]]]
    id_sets = [[2, 2], [9], [1], [1, 2], [0, 3], [R, 1], [], [5]]
    honest = [[13, 13], [0], [8], [1, 2], [3, 18], [7, 7], [], [15]]
    bits, st, raw = check(hs, table, commit_sets, id_sets, honest, 4)
    assert st == [0, 0, 3, 3, 1, 1, 0, 0]
    assert bits == [True, True, True] + [False] * 7 + [True]
    assert raw[-1] >> 3 == 0                                          # the pad bits of the last byte
    # wrong shares clear their own bit only; a group without commitments accepts zero alone; a share >= r never fails its group
    wrong = [[13, 14], [1], [8], [1, 2], [3, 18], [7, 7], [], [15 + R]]
    bits, st2, _ = check(hs, table, commit_sets, id_sets, wrong, 4)
    assert st2 == st
    assert bits == [True, False, False] + [False] * 7 + [False]
    # random polynomials, ragged sizes that straddle a byte of the bitmap, full-width ids
    rnd = random.Random(23)
    ts, ns = [1, 4, 0, 2], [3, 6, 2, 5]
    cs = [[rnd.randrange(1, R) for _ in range(t)] for t in ts]
    xs = [[rnd.randrange(1, R) for _ in range(n)] for n in ns]
    cm = [[oracle.sk_to_pk(a) for a in c] for c in cs]
    sh = [[poly_eval(c, x) for x in g] for c, g in zip(cs, xs)]
    assert check(hs, table, cm, xs, sh, 254)[:2] == ([True] * 16, [0] * 4)
    sh[1][2] = (sh[1][2] + 1) % R; sh[2][0] = 1; sh[3][4] = R - sh[3][4]
    want = [True] * 16
    for i in (3 + 2, 9, 11 + 4):
        want[i] = False
    assert check(hs, table, cm, xs, sh, 254)[:2] == (want, [0] * 4)
