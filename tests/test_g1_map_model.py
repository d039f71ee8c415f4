"""CPU-only: the model of the try-and-increment map (tests/g1_map_support.py) before any other test relies on it -- the
contracts' loop against the same map stated as a property, the facts the device code leans on (beta is never 0; the root taken is
the (p + 1) / 4 power, with no sign rule), the plain digests, and the helpers that prescribe run lengths."""
import hashlib
import random

from oracle.pyref import bn254 as ref
from tests import expander_support as X
from tests import g1_map_support as G

P = G.P


def test_minus_three_is_not_a_cube_so_beta_is_never_zero():
    """x^3 + 3 == 0 needs a cube root of -3; p = 1 mod 3, so the cubes are the (p - 1) / 3-th roots of unity's kernel"""
    assert P % 3 == 1 and P % 4 == 3
    assert pow(-3 % P, (P - 1) // 3, P) != 1
    # the group-theoretic reading: (x, 0) would have order 2, and the curve's order r is an odd prime
    assert ref.R % 2 == 1


def test_the_loop_and_the_property_agree():
    rnd = random.Random(254)
    xs = [rnd.randrange(P) for _ in range(300)] + [0, 1, P - 1, P - 2]
    for x0 in xs:
        pt, k = G.contract_loop(x0)
        assert G.holds(x0, pt, k), x0
        assert ref.g1_on_curve(pt)
        # the property refuses the other root, a later residue and a shorter run
        assert not G.holds(x0, (pt[0], -pt[1] % P), k)
        if k:
            assert not G.holds(x0, pt, k - 1)
    assert sum(G.run_of(x) for x in xs[:300]) in range(200, 420)        # mean run 1: 300 +- 3.5 sigma of sqrt(600)


def test_the_cap_yields_the_off_curve_point():
    d = G.digests_with_run(12, 1, at_least=True)[0]
    assert G.hash_to_g1(G.TAI_DIGEST, 0, d, cap=4) is None and G.hash_bytes(G.TAI_DIGEST, 0, d, cap=4) == bytes(64)
    assert not ref.g1_on_curve((0, 0))
    pt = G.hash_to_g1(G.TAI_DIGEST, 0, d, cap=13 + G.run_of(int.from_bytes(d, "big")))
    assert pt is not None and ref.g1_on_curve(pt)


def test_x0_reduces_any_length_as_one_big_endian_integer():
    assert [G.x0_of(G.TAI_DIGEST, 0, d) for d in G.EDGE_DIGESTS] == [P - 1, 0, 5, ((1 << 256) - 1) % P]
    for m in G.ODD_LENGTHS:
        v = 0
        for b in m:                                                    # byte-wise Horner
            v = (v * 256 + b) % P
        assert G.x0_of(G.TAI_DIGEST, 3, m) == v
    # p - 1 is itself a winner (beta = 2, a square for p = 7 mod 8): a search never steps from p - 1 to 0; p - 2 steps to p - 1
    assert G.run_of(P - 1) == 0 and G.contract_loop(P - 2)[0][0] in (P - 2, P - 1)


def test_plain_digests():
    m = b"try and increment"
    assert G.PLAIN[X.XMD_SHA256](m) == hashlib.sha256(m).digest()
    assert G.PLAIN[X.XMD_KECCAK256](b"") == bytes.fromhex("c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470")
    assert G.PLAIN[X.XMD_SHA3_256](m) == X.sha3_256(m) and G.PLAIN[X.XOF_SHAKE128](m) == X.shake128(m, 32) and G.PLAIN[X.XOF_SHAKE256](m) == X.shake256(m, 32)
    assert len({G.x0_of(G.TAI_HASH, xid, m) for xid in X.IDS}) == 5
    assert G.x0_of(G.TAI_HASH, X.XMD_KECCAK256, m) == int.from_bytes(X.keccak256(m), "big") % P


def test_prescribed_runs():
    for run in (0, 1, 2, 3, 5):
        for d in G.digests_with_run(run, 3):
            assert G.run_of(int.from_bytes(d, "big")) == run
    for n in (1, 63, 64, 65, 130):
        w = G.mixed_wave(n)
        assert len(w) == n == len(set(w))
        runs = [G.run_of(G.x0_of(G.TAI_DIGEST, 0, d)) for d in w]
        for lo in range(0, n, 64):
            assert max(runs[lo:lo + 64]) >= 12
        if n >= 63:
            assert {0, 1, 2, 3, 5} <= set(runs) and all(d in w for d in G.EDGE_DIGESTS)
    assert all(G.run_of(int.from_bytes(d, "big")) >= 3 for d in G.digests_with_run(3, 64, at_least=True))
