"""CPU-only: the lane functions of the threshold dealing side (bls-bn254_amd/csrc/threshold_deal.h) compiled for the host with
-DBN_CHECK, so every field operation asserts the lazy-limb interval discipline: the Horner evaluation of a group's polynomial
in Fr against Python integers, and "in the exponent" of G2 against the oracle's g2_mul / g2_add composed the same way and
against sk_to_pk(f(id)), at the bit counts a launch can have.  A test tool; the product has no CPU path."""
import ctypes
import random

import pytest

from tests import hostsim_build
from tests.helpers import b32, IDENT2, offsets_u32

u32p = ctypes.POINTER(ctypes.c_uint32)


@pytest.fixture(scope="module")
def hs():
    so = hostsim_build.build("threshold_deal_host.cpp", "libthresholddealhost.so")
    return ctypes.CDLL(so)


def poly_eval_mod(coeffs, x, R):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def fr_eval(hs, coef_sets, id_sets):
    coff, goff = offsets_u32([len(s) for s in coef_sets]), offsets_u32([len(s) for s in id_sets])
    n = int(goff[-1])
    out = ctypes.create_string_buffer(32 * max(n, 1))
    st = ctypes.create_string_buffer(len(id_sets))
    hs.hs_td_fr_eval(b"".join(b32(c) for s in coef_sets for c in s), coff.ctypes.data_as(u32p), b"".join(b32(x) for s in id_sets for x in s),
                     goff.ctypes.data_as(u32p), len(id_sets), out, st)
    return out.raw[:32 * n], list(st.raw), goff


def g2_eval(hs, commit_sets, id_sets, nbits):
    coff, goff = offsets_u32([len(s) for s in commit_sets]), offsets_u32([len(s) for s in id_sets])
    n = int(goff[-1])
    out = ctypes.create_string_buffer(128 * max(n, 1))
    st = ctypes.create_string_buffer(len(id_sets))
    hs.hs_td_g2_eval(b"".join(c for s in commit_sets for c in s), coff.ctypes.data_as(u32p), b"".join(b32(x) for s in id_sets for x in s),
                     goff.ctypes.data_as(u32p), len(id_sets), ctypes.c_int(nbits), out, st)
    return out.raw[:128 * n], list(st.raw), goff


def test_fr_horner_matches_python_integers(hs, pyref):
    R = pyref.R
    rnd = random.Random(1)
    ts = [0, 1, 2, 9, 2, 9]
    coef_sets = [[rnd.randrange(R) for _ in range(t)] for t in ts]
    coef_sets[3][4] = R - 1; coef_sets[3][8] = R - 1; coef_sets[4] = [0, R - 1]; coef_sets[5][0] = 0
    id_sets = [[1, 2, R - 1], [rnd.randrange(1, R), 7], [R - 1, 1, rnd.randrange(1, R)], [R - 1, 3, rnd.randrange(1, R), 3],
               [R - 1, R - 2], []]
    got, st, goff = fr_eval(hs, coef_sets, id_sets)
    assert st == [0] * len(ts)
    for g, (cs, xs) in enumerate(zip(coef_sets, id_sets)):
        for i, x in enumerate(xs):
            p = int(goff[g]) + i
            assert got[32 * p:32 * p + 32] == b32(poly_eval_mod(cs, x, R)), (g, i)


def test_fr_bad_scalars_mark_their_group_only(hs, pyref):
    R = pyref.R
    coef_sets = [[5, 6], [R, 1], [3], [4, 4, 4], [R + 1], [9]]
    id_sets = [[1, 2], [1, 2], [0, 5], [2, R, 3], [], [7, 7]]
    got, st, goff = fr_eval(hs, coef_sets, id_sets)
    assert st == [0, 1, 1, 1, 1, 0]
    assert got == b32(11) + b32(17) + bytes(32 * 7) + b32(9) * 2


def test_g2_horner_matches_the_oracle(hs, oracle, pyref):
    R = pyref.R
    rnd = random.Random(2)
    G2 = oracle.g2_generator()
    for nbits, ids in ((1, [1, 1]), (16, [1, 0x8001, 0xffff, 2]), (254, [R - 1, rnd.randrange(1 << 253, R)])):
        ts = [1, 2, 4]
        coef_sets = [[rnd.randrange(1, R) for _ in range(t)] for t in ts]
        commit_sets = [[oracle.g2_mul(G2, a) for a in cs] for cs in coef_sets]
        id_sets = [list(ids) for _ in ts]
        got, st, goff = g2_eval(hs, commit_sets, id_sets, nbits)
        assert st == [0, 0, 0]
        for g, (cs, cm) in enumerate(zip(coef_sets, commit_sets)):
            for i, x in enumerate(ids):
                p = int(goff[g]) + i
                acc = cm[-1]
                for c in reversed(cm[:-1]):
                    acc = oracle.g2_add(oracle.g2_mul(acc, x), c)
                assert got[128 * p:128 * p + 128] == acc, (nbits, g, i)
                assert acc == oracle.sk_to_pk(poly_eval_mod(cs, x, R)), (nbits, g, i)
        if nbits < 254:                                              # the same ids under a larger bit count: the same bytes
            for wider in (nbits + 1, 64, 254):
                assert g2_eval(hs, commit_sets, id_sets, wider)[0] == got, (nbits, wider)


def test_g2_marks_and_the_empty_polynomial(hs, oracle, pyref):
    from tests import synth
    R = pyref.R
    G2 = oracle.g2_generator()
    C = [oracle.g2_mul(G2, k) for k in (3, 5, 7)]
    off_curve = bytearray(C[1]); off_curve[127] ^= 1
    commit_sets = [C[:2], [], [C[0], bytes(off_curve)], [synth.NON_SUBGROUP_PK], C[:2], [b"\xff" * 128, C[2]], [C[2]], [IDENT2, C[0]]]
    id_sets = [[2, 2], [9], [1], [1, 2], [0, 3], [R, 1], [], [5]]
    got, st, goff = g2_eval(hs, commit_sets, id_sets, 4)
    assert st == [0, 0, 3, 3, 1, 1, 0, 0]
    # group 1 has no commitments (the identity, status 0); the last group's constant term is the identity: f = 3 x
    want = [oracle.sk_to_pk(3 + 5 * 2)] * 2 + [IDENT2] * 8 + [oracle.sk_to_pk(3 * 5)]
    assert got == b"".join(want)
