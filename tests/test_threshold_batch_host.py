"""CPU-only: the lane functions of the threshold combine over many groups (bls-bn254_amd/csrc/threshold_batch.h) compiled for the
host with -DBN_CHECK, so every field operation asserts the lazy-limb interval discipline: the segmented Lagrange coefficients,
the GLV scalar multiplication on one doubling chain, and a whole small batch against the oracle.  A test tool; the product has
no CPU path."""
import ctypes
import random

import pytest

from tests import hostsim_build
from tests.helpers import b32, glv_lambda, IDENT1, offsets_u32

u32p = ctypes.POINTER(ctypes.c_uint32)


@pytest.fixture(scope="module")
def hs():
    so = hostsim_build.build("threshold_batch_host.cpp", "libthresholdbatchhost.so")
    return ctypes.CDLL(so)


def lagrange(hs, id_sets):
    off = offsets_u32([len(s) for s in id_sets])
    n = int(off[-1])
    out = ctypes.create_string_buffer(32 * max(n, 1))
    bad = ctypes.create_string_buffer(len(id_sets))
    hs.hs_thb_lagrange(b"".join(b"".join(s) for s in id_sets), off.ctypes.data_as(u32p), len(id_sets), out, bad)
    return out.raw[:32 * n], list(bad.raw), off


def test_segmented_lagrange_matches_the_oracle_per_group(hs, oracle, pyref):
    R = pyref.R
    rnd = random.Random(1)
    sizes = [1, 2, 3, 7, 1, 0, 20, 33, 0, 5]
    id_sets = [[b32(x) for x in rnd.sample(range(1, 1 << 16), k)] for k in sizes]
    id_sets[3] = [b32(x) for x in (1, 2, R - 1, rnd.randrange(1, R), rnd.randrange(1, R), R - 2, 3)]     # full-range ids
    id_sets[6] = [b32(rnd.randrange(1, R)) for _ in range(20)]
    id_sets[9] = list(id_sets[3][:5])                                # the same ids as another group: fine
    got, bad, off = lagrange(hs, id_sets)
    assert bad == [0] * len(sizes)
    for g, s in enumerate(id_sets):
        lo, hi = int(off[g]), int(off[g + 1])
        assert got[32 * lo:32 * hi] == (oracle.fr_lagrange_at_zero(b"".join(s), len(s)) if s else b""), g


def test_duplicates_count_inside_a_group_only(hs, pyref):
    R = pyref.R
    a, b, c = b32(5), b32(R - 7), b32(11)
    id_sets = [[a, b, c], [a, b], [a, c, a], [b32(0), a], [b32(R), c], [c], [b, b]]
    _, bad, _ = lagrange(hs, id_sets)
    assert bad == [0, 0, 1, 1, 1, 0, 1]


def test_glv_multiplication_matches_the_oracle(hs, oracle, pyref):
    R, lam = pyref.R, glv_lambda()
    rnd = random.Random(2)
    G1 = oracle.g1_generator()
    out = ctypes.create_string_buffer(64)
    edge = [0, 1, R - 1, lam, lam + 1, lam - 1, 2 ** 127, 2 ** 128 - 1, 2, R - 2]
    pts = [oracle.g1_mul(G1, rnd.randrange(1, R)) for _ in range(8)]
    seen = set()
    for j, k in enumerate(edge + [rnd.randrange(R) for _ in range(1000)]):
        p = pts[j % len(pts)]
        fl = hs.hs_thb_smul(p, b32(k), out)
        assert fl & 1
        seen.add(fl >> 1)
        assert out.raw == oracle.g1_mul(p, k), hex(k)
    assert {f & 2 for f in seen} == {0, 2}, "both signs of k2 (glv_split gives no negative k1 for a canonical scalar)"
    assert {f >> 2 for f in seen} == {0, 1, 2, 3}, "odd and even halves, in every combination"
    # explicit halves: every combination of the two signs, magnitudes up to 2^127 and 2^128 - 1, zero and even halves
    mags = [0, 1, 2, 2 ** 127, 2 ** 127 + 1, 2 ** 128 - 1, 2 ** 128 - 2] + [rnd.randrange(2 ** 128) for _ in range(12)]
    for j in range(120):
        k1, k2, neg = mags[j % len(mags)], mags[(j * 7 + 3) % len(mags)], j & 3
        p = pts[j % len(pts)]
        hs.hs_thb_smul_halves(p, k1.to_bytes(16, "big"), k2.to_bytes(16, "big"), neg, out)
        k = ((-k1 if neg & 1 else k1) + (-k2 if neg & 2 else k2) * lam) % R
        assert out.raw == oracle.g1_mul(p, k), (hex(k1), hex(k2), neg)
    for k in edge + [rnd.randrange(R) for _ in range(20)]:             # the identity stays the identity
        assert hs.hs_thb_smul(IDENT1, b32(k), out) & 1
        assert out.raw == IDENT1
    # an undecodable or off-curve point is replaced (flag clear), never multiplied
    off_curve = bytearray(pts[0]); off_curve[63] ^= 1
    assert hs.hs_thb_smul(bytes(off_curve), b32(7), out) & 1 == 0
    assert hs.hs_thb_smul(b"\xff" * 64, b32(7), out) & 1 == 0


def test_whole_small_batch_matches_threshold_combine_per_group(hs, oracle, pyref):
    R = pyref.R
    rnd = random.Random(3)
    sizes = [0, 1, 2, 7, 33, 3, 2, 2, 2]
    H = oracle.g1_mul(oracle.g1_generator(), rnd.randrange(1, R))
    id_sets = [[b32(rnd.randrange(1, R)) for _ in range(k)] for k in sizes]
    sig_sets = [[oracle.g1_mul(H, rnd.randrange(1, R)) for _ in range(k)] for k in sizes]
    sig_sets[3][2] = IDENT1                                          # an identity share contributes nothing
    id_sets[5][1] = id_sets[5][0]                                    # group 5: repeated id
    bad_pt = bytearray(sig_sets[6][1]); bad_pt[63] ^= 1
    sig_sets[6][1] = bytes(bad_pt)                                   # group 6: off the curve
    sig_sets[7][0] = b"\xff" * 64                                    # group 7: does not decode
    id_sets[8][0] = b32(0); sig_sets[8][1] = b"\xff" * 64            # group 8: both; the scalar error wins
    off = offsets_u32(sizes)
    ng = len(sizes)
    out = ctypes.create_string_buffer(64 * ng)
    st = ctypes.create_string_buffer(ng)
    hs.hs_thb_combine(b"".join(b"".join(s) for s in id_sets), b"".join(b"".join(s) for s in sig_sets), off.ctypes.data_as(u32p), ng, out, st)
    assert list(st.raw) == [0, 0, 0, 0, 0, 1, 2, 2, 1]
    for g in range(ng):
        if g >= 5:
            want = IDENT1
        elif sizes[g] == 0:
            want = IDENT1
        else:
            want = oracle.threshold_combine(b"".join(id_sets[g]), b"".join(sig_sets[g]), sizes[g])
        assert out.raw[64 * g:64 * g + 64] == want, g
