"""CPU-only: the multi-scalar multiplication lane functions (bls-bn254_amd/csrc/msm.h) compiled for the host with -DBN_CHECK, so
every field operation asserts the lazy-limb interval discipline: signed-digit recoding, the complete mixed addition, and the
recode -> sort -> bucket levels -> reduce -> Horner pipeline against the oracle.  A test tool; the product has no CPU path."""
import ctypes
import random

import pytest

from tests import hostsim_build
from tests.helpers import b32, glv_lambda, IDENT1, IDENT2


@pytest.fixture(scope="module")
def hs():
    so = hostsim_build.build("msm_host.cpp", "libmsmhost.so")
    return ctypes.CDLL(so)


def digits(hs, k, c, half):
    d = (ctypes.c_int32 * 200)()
    neg = ctypes.c_int(0)
    W = hs.hs_msm_digits(b32(k), c, half, d, ctypes.byref(neg))
    return [d[i] for i in range(W)], neg.value


def test_recoding_reconstructs_every_scalar_and_glv_half(hs, pyref):
    R, lam = pyref.R, glv_lambda()
    rnd = random.Random(1)
    ks = [0, 1, R - 1, (R - 1) // 2, 2 ** 127, 2 ** 128 - 1, lam, lam + 1, lam - 1, 2, R - 2] + [rnd.randrange(R) for _ in range(10000)]
    for c in range(2, 17):
        sample = ks if c in (2, 15, 16) else ks[:11] + ks[11::20]
        for k in sample:
            d, _ = digits(hs, k, c, -1)
            assert len(d) == (254 + c) // c
            assert all(abs(x) <= 1 << (c - 1) for x in d)
            assert sum(x << (c * j) for j, x in enumerate(d)) == k, (c, hex(k))
            (d1, n1), (d2, n2) = digits(hs, k, c, 0), digits(hs, k, c, 1)
            k1 = sum(x << (c * j) for j, x in enumerate(d1))        # |k1|, |k2|; the halves' signs come back separately
            k2 = sum(x << (c * j) for j, x in enumerate(d2))
            k1, k2 = (-k1 if n1 else k1), (-k2 if n2 else k2)
            assert all(abs(x) <= 1 << (c - 1) for x in d1 + d2)
            assert abs(k1) <= 2 ** 128 and abs(k2) <= 2 ** 128
            assert (k1 + k2 * lam - k) % R == 0, (c, hex(k))


def test_mixed_addition_matches_the_oracle(hs, oracle, pyref):
    rnd = random.Random(2)
    G1, G2 = oracle.g1_generator(), oracle.g2_generator()
    o1, o2 = ctypes.create_string_buffer(64), ctypes.create_string_buffer(128)
    for _ in range(20):
        p, q = oracle.g1_mul(G1, rnd.randrange(1, pyref.R)), oracle.g1_mul(G1, rnd.randrange(1, pyref.R))
        neg = oracle.g1_mul(q, pyref.R - 1)
        for a, b in ((p, q), (q, q), (neg, q), (IDENT1, q)):
            hs.hs_msm_madd_g1(a, b, o1)
            assert o1.raw == oracle.g1_add(a, b)
        p2, q2 = oracle.g2_mul(G2, rnd.randrange(1, pyref.R)), oracle.g2_mul(G2, rnd.randrange(1, pyref.R))
        neg2 = oracle.g2_mul(q2, pyref.R - 1)
        for a, b in ((p2, q2), (q2, q2), (neg2, q2), (IDENT2, q2)):
            hs.hs_msm_madd_g2(a, b, o2)
            assert o2.raw == oracle.g2_add(a, b)


def test_host_pipeline_matches_the_oracle_fold(hs, oracle, pyref):
    rnd = random.Random(3)
    R, lam = pyref.R, glv_lambda()
    G1, G2 = oracle.g1_generator(), oracle.g2_generator()
    n = 200
    pts = [oracle.g1_mul(G1, rnd.randrange(1, R)) for _ in range(n)]
    pts[5] = IDENT1
    pts[7] = pts[6]
    ks = [rnd.randrange(R) for _ in range(n)]
    ks[:8] = [0, 1, R - 1, lam, 2 ** 127, 2 ** 128 - 1, 7, 7]
    want = IDENT1
    for p, k in zip(pts, ks):
        want = oracle.g1_add(want, oracle.g1_mul(p, k))
    out = ctypes.create_string_buffer(64)
    for c in (2, 5, 8, 13):
        hs.hs_msm_g1(b"".join(pts), b"".join(map(b32, ks)), ctypes.c_size_t(n), c, out)
        assert out.raw == want, c
    m = 40
    q = [oracle.g2_mul(G2, rnd.randrange(1, R)) for _ in range(m)]
    kq = [rnd.randrange(R) for _ in range(m)]
    want2 = IDENT2
    for p, k in zip(q, kq):
        want2 = oracle.g2_add(want2, oracle.g2_mul(p, k))
    out2 = ctypes.create_string_buffer(128)
    for c in (3, 7):
        hs.hs_msm_g2(b"".join(q), b"".join(map(b32, kq)), ctypes.c_size_t(m), c, out2)
        assert out2.raw == want2, c
