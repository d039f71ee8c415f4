"""CPU-only: the unit-coefficient line pairs of the prepared-key verify path (pairing.h: line_pair_expand_unit, fp2_inv4,
miller_unit_coords, miller_loop_prepared_unit), compiled for the host with -DBN_CHECK so that every multiply asserts the
lazy-limb interval discipline, against the oracle; the integer argument that the key's x-coefficient b3 never vanishes; and
the executed-MAD count of the new loop.  A test tool; the product has no CPU path."""
import ctypes
import random

import pytest

from tests import hostsim_build
from tests.helpers import IDENT1

GT_ONE = (1).to_bytes(32, "big") + bytes(352)
PARENT_LOOP_MADS = 1371816          # miller_loop_prepared, profiles/r03_executed_mads.json
PAIR_SAVING = 88 * 810              # 324 (the scaling of T2) + 486 (one Fp2 product of the sparse multiplication) per line pair


@pytest.fixture(scope="module")
def hs():
    so = hostsim_build.build("unit_pairs_host.cpp", "libunitpairs.so")
    return ctypes.CDLL(so)


def unit_verify(hs, sig, h, pk, z, h_identity=False):
    gt = ctypes.create_string_buffer(384)
    counts = (ctypes.c_double * 12)()
    zeros = hs.hs_unit_verify(sig, h, pk, z, 1 if h_identity else 0, gt, counts)
    return zeros, gt.raw, [int(c) for c in counts]


def mads(c):
    mul, sqr, dot, _norm, _lcs, terms = c
    return 162 * mul + 126 * sqr + 243 * dot + 9 * terms


def test_unit_loop_equals_the_oracle_after_the_final_exponentiation(hs, oracle, pyref):
    """final_exponentiation(miller_loop_prepared_unit) == the oracle's final exponentiation of the textbook Miller value, byte for
    byte, for H = (z x : z y : z) with several z; exactly one for a correctly signed tuple; the lane with H = identity; a key
    outside the subgroup (the same formulas; its validity byte is what masks it)."""
    from tests import synth
    rnd = random.Random(41)
    G1, G2 = oracle.g1_generator(), oracle.g2_generator()
    neg_g2 = pyref.g2_to_bytes(pyref.g2_neg(pyref.G2_GEN))
    for trial in range(3):
        sk = rnd.randrange(1, pyref.R)
        pk = oracle.g2_mul(G2, sk)
        h = oracle.g1_mul(G1, rnd.randrange(1, pyref.R))
        good = oracle.g1_mul(h, sk)                                   # sk * H: the signature of the message hashing to H
        other = oracle.g1_mul(G1, rnd.randrange(1, pyref.R))
        for sig, valid in ((good, True), (other, False)):
            want = oracle.final_exponentiation(oracle.multi_miller_loop(sig + h, neg_g2 + pk, 2), 1)
            assert (want == GT_ONE) == valid
            for z in (1, 2, 5, 7) if trial == 0 else (1, 3):
                zeros, got, _ = unit_verify(hs, sig, h, pk, z)
                assert zeros == 0 and got == want, (trial, valid, z)
        # H(msg) = identity: X = Z = 0, the lane keeps scale 1 and a zero v-coefficient
        want = oracle.final_exponentiation(oracle.multi_miller_loop(good + IDENT1, neg_g2 + pk, 2), 1)
        zeros, got, _ = unit_verify(hs, good, h, pk, 1, h_identity=True)
        assert zeros == 0 and got == want and got != GT_ONE
        assert hs.hs_unit_slot2_is_one(pk) == 1
    # an invalid key: on the curve, outside the subgroup.  Its table is well defined and the loop is the same polynomial identity.
    bad = synth.NON_SUBGROUP_PK
    assert oracle.g2_check_batch(bad, 1) != b"\x01"
    sig, h = oracle.g1_mul(G1, 5), oracle.g1_mul(G1, 7)
    zeros, got, _ = unit_verify(hs, sig, h, bad, 3)
    assert zeros == 0
    assert got == oracle.final_exponentiation(oracle.multi_miller_loop(sig + h, neg_g2 + bad, 2), 1)
    assert hs.hs_unit_slot2_is_one(bad) == 1


def test_quad_and_wave_loops_read_the_unit_table_unchanged(hs, oracle, pyref):
    """tri.h (k_miller_tri_prepared) and wide.h (k_miller_wide_prepared) keep reading the 162-limb entries with the unscaled
    coordinate values: their values change by an Fp2 factor per step, which the final exponentiation removes."""
    rnd = random.Random(43)
    G1, G2 = oracle.g1_generator(), oracle.g2_generator()
    neg_g2 = pyref.g2_to_bytes(pyref.g2_neg(pyref.G2_GEN))
    g1 = ctypes.create_string_buffer(384); g2 = ctypes.create_string_buffer(384)
    sk = rnd.randrange(1, pyref.R)
    pk = oracle.g2_mul(G2, sk)
    h = oracle.g1_mul(G1, rnd.randrange(1, pyref.R))
    for sig, z in ((oracle.g1_mul(h, sk), 1), (oracle.g1_mul(G1, rnd.randrange(1, pyref.R)), 3)):
        want = oracle.final_exponentiation(oracle.multi_miller_loop(sig + h, neg_g2 + pk, 2), 1)
        assert hs.hs_unit_tri_wide(sig, h, pk, z, g1, g2) == 0
        assert g1.raw == want and g2.raw == want
        assert (want == GT_ONE) == (z == 1)


def test_fp2_inv4_shares_one_inversion(hs, pyref):
    P = pyref.P
    rnd = random.Random(42)

    def enc(v):
        return v[0].to_bytes(32, "big") + v[1].to_bytes(32, "big")
    edge = [(0, 0), (1, 0), (0, 1), (P - 1, P - 1), (0, P - 1), (2, 0)]
    for k in range(12):
        vals = [(rnd.randrange(P), rnd.randrange(P)) for _ in range(4)]
        if k < 6:
            vals[k % 4] = edge[k]
        if k == 6:
            vals = [(0, 0)] * 4
        if k == 7:
            vals[1] = vals[3] = (0, 0)
        assert hs.hs_fp2_inv4_matches(b"".join(enc(v) for v in vals)) == 1, vals


def test_key_line_x_coefficient_never_vanishes(hs, pyref):
    """b3 of a tangent is -6 x_T^2 z_T^2: zero only for T = O or x_T = 0 (a point of order 3, not in the r-torsion).  b3 of a chord
    through T and the added point Q' is -4 (y_Q' z_T^3 - y_T): zero iff T has the affine y of Q', and on this j = 0 twist that is
    T in {Q', phi Q', phi^2 Q'} with phi(x, y) = (omega x, y), which acts on G2 as a cube root of unity lambda mod r.  With
    T = m_T Q and Q' = m_Q Q the condition is m_T != m_Q {1, lambda, lambda^2} and m_T != 0 (mod r), walked here over the loop's
    own digits (ate_naf_digit) with integers: the NAF additions (m_Q = +-1) and the two Frobenius additions (m_Q = p, -p^2)."""
    r, p = pyref.R, pyref.P
    lam = next(c for c in (pow(g, (r - 1) // 3, r) for g in range(2, 50)) if c != 1)
    assert (lam * lam + lam + 1) % r == 0
    n = hs.hs_ate_naf_len()
    digits = [hs.hs_ate_naf_digit(j) for j in range(n)]
    assert sum(d << j for j, d in enumerate(digits)) == 6 * pyref.X + 2 and digits[n - 1] == 1
    lines = []

    def chord(m, mq):
        assert m % r != 0
        for c in (1, lam, lam * lam):
            assert (m - mq * c) % r != 0, (len(lines), mq)
        lines.append("add")
        return (m + mq) % r
    m = 1
    for j in range(n - 2, -1, -1):
        assert m % r != 0                                        # tangent: T is not O (and a point of order 3 is not in the r-torsion)
        lines.append("dbl")
        m = 2 * m % r
        if digits[j]:
            m = chord(m, digits[j])
    assert m == (6 * pyref.X + 2) % r
    m = chord(m, p % r)
    m = chord(m, -p * p % r)
    assert len(lines) == 88 and lines.count("dbl") == 65
    assert (m + p ** 3) % r == 0                                # the walk itself: 6x + 2 + p - p^2 + p^3 = 0 (mod r)


def test_executed_mads_of_the_unit_loop(hs, oracle, pyref):
    """The operation counters of scripts/executed_mads.py applied to the new loop: at most the parent's count less 810 per line
    pair; the prologue (nine products and what fp_inv multiplies around its divstep recurrence) is counted on its own."""
    G1, G2 = oracle.g1_generator(), oracle.g2_generator()
    _, _, c = unit_verify(hs, oracle.g1_mul(G1, 3), oracle.g1_mul(G1, 4), oracle.g2_mul(G2, 5), 1)
    loop, prologue = mads(c[:6]), mads(c[6:])
    print("unit loop: %d executed MADs (%s), prologue %d (%s)" % (loop, c[:6], prologue, c[6:]))
    assert loop <= PARENT_LOOP_MADS - PAIR_SAVING
    assert prologue <= 14 * 162
