"""GPU tests (MI355X) of the multi-scalar multiplication sum_i [k_i] P_i (blsbn254_g1_msm / blsbn254_g2_msm): small cases against
the oracle's Mul<Scalar> and Add folded in Python, every window width, the GLV split boundaries, identities and cancellations,
points outside the G2 r-torsion, the error mapping, and large cases (2^20 G1 terms, 2^18 G2 terms) in closed form:
with P_i = [a_i] G, sum_i [k_i] P_i = [sum_i k_i a_i mod r] G."""
import random

import pytest

from tests import synth
from tests.gpu_support import eng, M
from tests.helpers import b32, glv_lambda, IDENT1, IDENT2

pytestmark = pytest.mark.gpu


def fold(oracle, pts, ks, g2=False):
    sz = 128 if g2 else 64
    mul, add = (oracle.g2_mul, oracle.g2_add) if g2 else (oracle.g1_mul, oracle.g1_add)
    acc = IDENT2 if g2 else IDENT1
    for i, k in enumerate(ks):
        acc = add(acc, mul(pts[sz * i:sz * i + sz], k))
    return acc


def rand_g1(oracle, pyref, rnd, n):
    G1 = oracle.g1_generator()
    return b"".join(oracle.g1_mul(G1, rnd.randrange(1, pyref.R)) for _ in range(n))


def rand_g2(oracle, pyref, rnd, n):
    G2 = oracle.g2_generator()
    return b"".join(oracle.g2_mul(G2, rnd.randrange(1, pyref.R)) for _ in range(n))


def edge_scalars(pyref):
    R, lam = pyref.R, glv_lambda()
    return [0, 1, R - 1, (R - 1) // 2, 2 ** 127, 2 ** 128 - 1, lam, lam + 1, 2, R - 2, 2 ** 64, lam - 1]


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 1000, 4097])
def test_g1_msm_random_vs_oracle(eng, oracle, pyref, n):
    rnd = random.Random(100 + n)
    pts = rand_g1(oracle, pyref, rnd, n)
    ks = [rnd.randrange(pyref.R) for _ in range(n)]
    assert eng.g1_msm(pts, b"".join(map(b32, ks)), n) == fold(oracle, pts, ks)


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 1000])
def test_g2_msm_random_vs_oracle(eng, oracle, pyref, n):
    rnd = random.Random(200 + n)
    pts = rand_g2(oracle, pyref, rnd, n)
    ks = [rnd.randrange(pyref.R) for _ in range(n)]
    assert eng.g2_msm(pts, b"".join(map(b32, ks)), n) == fold(oracle, pts, ks, g2=True)


def test_every_window_width_agrees(eng, oracle, pyref):
    rnd = random.Random(3)
    n = 300
    p1, p2 = rand_g1(oracle, pyref, rnd, n), rand_g2(oracle, pyref, rnd, 40)
    ks = [rnd.randrange(pyref.R) for _ in range(n)]
    ks[:len(edge_scalars(pyref))] = edge_scalars(pyref)
    sc = b"".join(map(b32, ks))
    want1, want2 = fold(oracle, p1, ks), fold(oracle, p2, ks[:40], g2=True)
    before = eng.msm_stats()["bucket_calls"]
    try:
        for c in range(2, 17):
            eng.set_msm_window(c)
            assert eng.g1_msm(p1, sc, n) == want1, c
            assert eng.g2_msm(p2, sc[:32 * 40], 40) == want2, c
    finally:
        eng.set_msm_window(0)
    st = eng.msm_stats()
    assert st["bucket_calls"] - before == 30 and st["entries"] > 0 and st["chunks"] > 0


def test_window_argument_checked(eng, M):
    for bad in (1, 17, -1):
        with pytest.raises(M.Bn254Error):
            eng.set_msm_window(bad)
    eng.set_msm_window(0)


def test_edge_scalars_each(eng, oracle, pyref):
    rnd = random.Random(4)
    P, Q = rand_g1(oracle, pyref, rnd, 1), rand_g2(oracle, pyref, rnd, 1)
    for k in edge_scalars(pyref):
        assert eng.g1_msm(P, b32(k), 1) == oracle.g1_mul(P, k), hex(k)
        assert eng.g2_msm(Q, b32(k), 1) == oracle.g2_mul(Q, k), hex(k)
    ks = edge_scalars(pyref)
    pts = rand_g1(oracle, pyref, rnd, len(ks))
    assert eng.g1_msm(pts, b"".join(map(b32, ks)), len(ks)) == fold(oracle, pts, ks)


def test_identities_cancellations_and_repeats(eng, oracle, pyref):
    rnd = random.Random(5)
    P = rand_g1(oracle, pyref, rnd, 1)
    negP = oracle.g1_mul(P, pyref.R - 1)
    k = rnd.randrange(pyref.R)
    # identity points among the terms
    pts = rand_g1(oracle, pyref, rnd, 10)
    pts = pts[:64 * 3] + IDENT1 + pts[64 * 4:]
    ks = [rnd.randrange(pyref.R) for _ in range(10)]
    assert eng.g1_msm(pts, b"".join(map(b32, ks)), 10) == fold(oracle, pts, ks)
    assert eng.g1_msm(IDENT1 * 5, b"".join(map(b32, ks[:5])), 5) == IDENT1
    # the same point with the same scalar: a doubling inside a bucket
    assert eng.g1_msm(P * 7, b32(k) * 7, 7) == oracle.g1_mul(P, 7 * k % pyref.R)
    # P and -P with the same scalar: an identity bucket, an identity result
    assert eng.g1_msm(P + negP, b32(k) * 2, 2) == IDENT1
    assert eng.g1_msm(P + negP + P, b32(k) * 3, 3) == oracle.g1_mul(P, k)
    # all scalars zero
    assert eng.g1_msm(pts, bytes(32 * 10), 10) == IDENT1
    Q = rand_g2(oracle, pyref, rnd, 1)
    assert eng.g2_msm(Q * 5, b32(k) * 5, 5) == oracle.g2_mul(Q, 5 * k % pyref.R)
    assert eng.g2_msm(Q + IDENT2 + oracle.g2_mul(Q, pyref.R - 1), b32(k) * 3, 3) == IDENT2
    assert eng.g2_msm(Q * 4, bytes(128), 4) == IDENT2


def test_g2_outside_the_r_torsion(eng, oracle, pyref):
    rnd = random.Random(6)
    pts = rand_g2(oracle, pyref, rnd, 6)
    pts = pts[:128 * 2] + synth.NON_SUBGROUP_PK + pts[128 * 3:]
    ks = [rnd.randrange(pyref.R) for _ in range(6)]
    want = fold(oracle, pts, ks, g2=True)
    assert eng.g2_msm(pts, b"".join(map(b32, ks)), 6) == want
    for c in (3, 8, 13):
        eng.set_msm_window(c)
        try:
            assert eng.g2_msm(pts, b"".join(map(b32, ks)), 6) == want
        finally:
            eng.set_msm_window(0)


def test_n1_equals_mul_batch_and_n0_is_identity(eng, oracle, pyref):
    rnd = random.Random(7)
    P, Q = rand_g1(oracle, pyref, rnd, 1), rand_g2(oracle, pyref, rnd, 1)
    k = b32(rnd.randrange(pyref.R))
    assert eng.g1_msm(P, k, 1) == eng.g1_mul_batch(P, k, 1)
    assert eng.g2_msm(Q, k, 1) == eng.g2_mul_batch(Q, k, 1)
    assert eng.g1_msm(b"", b"", 0) == IDENT1
    assert eng.g2_msm(b"", b"", 0) == IDENT2


def test_errors(eng, oracle, pyref, M):
    rnd = random.Random(8)
    pts = bytearray(rand_g1(oracle, pyref, rnd, 5))
    sc = b"".join(b32(rnd.randrange(pyref.R)) for _ in range(5))
    bad = bytearray(pts); bad[64 * 2 + 63] ^= 1                         # y changed: off the curve
    with pytest.raises(M.InvalidG1Bytes) as ei:
        eng.g1_msm(bytes(bad), sc, 5)
    assert "element 2" in eng._lib.blsbn254_last_error(eng._ctx).decode()
    with pytest.raises(M.InvalidScalarBytes):
        eng.g1_msm(bytes(pts), sc[:32 * 3] + b32(pyref.R) + sc[32 * 4:], 5)
    q = bytearray(rand_g2(oracle, pyref, rnd, 3))
    qs = sc[:96]
    qb = bytearray(q); qb[128 + 127] ^= 1
    with pytest.raises(M.InvalidG2Bytes):
        eng.g2_msm(bytes(qb), qs, 3)
    with pytest.raises(M.InvalidScalarBytes):
        eng.g2_msm(bytes(q), qs[:32] + b"\xff" * 32 + qs[64:], 3)
    assert eng.g1_msm(bytes(pts), sc, 5) == fold(oracle, bytes(pts), [int.from_bytes(sc[32 * i:32 * i + 32], "big") for i in range(5)])


# ---------------------------------------------------------------- large cases in closed form
def _closed_form(eng, oracle, pyref, n, ks_fn, pts_equal=False, g2=False, seed=0):
    rnd = random.Random(seed)
    R = pyref.R
    gen = oracle.g2_generator() if g2 else oracle.g1_generator()
    sz = 128 if g2 else 64
    a = [rnd.randrange(1, R)] * n if pts_equal else [rnd.randrange(1, R) for _ in range(n)]
    ab = b"".join(map(b32, a))
    pts = (eng.g2_mul_batch if g2 else eng.g1_mul_batch)(gen * n, ab, n)
    mul = oracle.g2_mul if g2 else oracle.g1_mul
    for i in (0, 1, n // 2, n - 1):
        assert pts[sz * i:sz * i + sz] == mul(gen, a[i])
    ks = ks_fn(rnd, n)
    msm = eng.g2_msm if g2 else eng.g1_msm
    got = msm(pts, b"".join(map(b32, ks)), n)
    assert got == mul(gen, sum(k * x for k, x in zip(ks, a)) % R)
    ks2 = list(ks); ks2[n // 3] = (ks2[n // 3] + 1) % R                  # one scalar flipped: the output follows
    got2 = msm(pts, b"".join(map(b32, ks2)), n)
    assert got2 != got and got2 == mul(gen, sum(k * x for k, x in zip(ks2, a)) % R)


def test_g1_large_random(eng, oracle, pyref):
    _closed_form(eng, oracle, pyref, 1 << 20, lambda rnd, n: [rnd.randrange(pyref.R) for _ in range(n)], seed=11)


def test_g1_large_equal_scalars(eng, oracle, pyref):
    def ks(rnd, n):
        k = rnd.randrange(pyref.R)
        return [k] * n
    _closed_form(eng, oracle, pyref, 1 << 20, ks, seed=12)


def test_g1_large_equal_points(eng, oracle, pyref):
    _closed_form(eng, oracle, pyref, 1 << 20, lambda rnd, n: [rnd.randrange(pyref.R) for _ in range(n)], pts_equal=True, seed=13)


def test_g2_large_random(eng, oracle, pyref):
    _closed_form(eng, oracle, pyref, 1 << 18, lambda rnd, n: [rnd.randrange(pyref.R) for _ in range(n)], g2=True, seed=14)
