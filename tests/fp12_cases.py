"""Arbitrary Fp12 inputs for the calls that take an Fp12 value from the caller (final_exponentiation, gt_mul_batch, gt_pow_batch,
aggregate_finish): named edge cases, seeded random values, their final exponentiations by the oracle (computed once per run), and
the map that tiles them over a batch without a period.  A support module: the CPU test of the cases and the GPU tests import it."""
import random
from collections import OrderedDict

import numpy as np

from tests.helpers import EDGE_COEFFS, b32

D = 251                                   # distinct values per run: a prime, so that the tiling below has no short period
ZERO = 0                                  # the index of the zero case in values()
N_NAMED = 35                              # values()[N_NAMED:] are plain random values: neither zero nor in a subfield
ZERO_GT = bytes(384)
ONE_GT = b32(1) + bytes(352)
# the named cases that lie in Fp6 or in w Fp6: f^(p^6 - 1) is 1 or -1 there, so the easy part sends them to the identity
SUBFIELD = ("one", "minus_one", "fp", "fp2", "fp6", "w_fp6") + tuple("mono_%d" % k for k in range(1, 12))


def _fp12(coeffs):
    """twelve coefficients in Gt::to_repr order (c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2, each c0 then c1)"""
    assert len(coeffs) == 12
    return b"".join(b32(c) for c in coeffs)


def _inverse_source(pyref):
    rnd = random.Random(0xf12 + 1)
    return _fp12([rnd.randrange(pyref.P) for _ in range(12)])


def inverse_pair(oracle, pyref):
    """(x, x^-1) with x^-1 == named_cases()["inverse"]"""
    x = _inverse_source(pyref)
    return x, oracle.field_op_batch(50, x, None, 1)


def named_cases(oracle, pyref):
    """name -> 384 bytes, in a fixed order; the same bytes on every call"""
    P = pyref.P
    rnd = random.Random(0xf12)
    r = lambda k: [rnd.randrange(1, P) for _ in range(k)]
    c = OrderedDict()
    c["zero"] = ZERO_GT
    c["one"] = ONE_GT
    c["minus_one"] = _fp12([P - 1] + [0] * 11)
    c["fp"] = _fp12(r(1) + [0] * 11)
    c["fp2"] = _fp12(r(2) + [0] * 10)
    c["fp6"] = _fp12(r(6) + [0] * 6)                       # c1 = 0
    c["w_fp6"] = _fp12([0] * 6 + r(6))                     # c0 = 0
    c["all_p_minus_1"] = _fp12([P - 1] * 12)
    for k in range(1, 12):                                 # the twelve unit monomials: "one" is the first
        c["mono_%d" % k] = _fp12([int(j == k) for j in range(12)])
    for k in range(12):
        v = r(12); v[k] = 0
        c["hole_%d" % k] = _fp12(v)
    edge = [e for e in EDGE_COEFFS if e not in (2, P - 2, (P + 1) // 2, (P - 1) // 2)]
    c["edges"] = _fp12(edge[:12])                          # 0, 1, p - 1, 2^29, 2^29 - 1, 2^58, 2^232, 2^232 - 1, 2^253, 2^253 - 1, p // 3, 3
    g1 = oracle.g1_mul(oracle.g1_generator(), rnd.randrange(1, pyref.R))
    g2 = oracle.g2_mul(oracle.g2_generator(), rnd.randrange(1, pyref.R))
    c["miller"] = oracle.miller_loop_batch(g1, g2, 1)
    c["gt"] = oracle.pairing_batch(g1, g2, 1)
    c["inverse"] = inverse_pair(oracle, pyref)[1]
    assert len(c) == N_NAMED and all(len(v) == 384 for v in c.values())
    return c


_cache = {}


def values(oracle, pyref, d=D):
    """(names, vals, fes): the named cases followed by seeded random Fp12 values, d distinct values in all (names[i] is None for
    the random ones), and oracle.final_exponentiation of each.  Computed on the first call of a run; callers do not change them."""
    if d not in _cache:
        named = named_cases(oracle, pyref)
        names, vals = list(named), list(named.values())
        rnd = random.Random(0xf12 + 2)
        while len(vals) < d:
            v = _fp12([rnd.randrange(pyref.P) for _ in range(12)])
            if v not in vals:
                names.append(None); vals.append(v)
        assert len(set(vals)) == d and names[ZERO] == "zero"
        fe = oracle.final_exponentiation(b"".join(vals), d)
        _cache[d] = (names, vals, [fe[384 * i:384 * i + 384] for i in range(d)])
    return _cache[d]


def zero_positions(n):
    """where spread() puts the zero case: the first position, the last of the first quarter (q = ceil(n / 4); the lane of
    k_fe_inv4 whose fourth tuple is past the end when n % 4 != 0), the last position"""
    q = (n + 3) // 4
    return sorted({0, q - 1, n - 1})


def partners(n, pos):
    """the positions that share one inversion with `pos` in k_fe_inv4 (pos +- k q inside 0 .. n), the other zero positions left
    out: with n % 4 == 0 the positions q - 1 and n - 1 are in one lane, which then inverts two zeros beside two other values"""
    q = (n + 3) // 4
    zs = zero_positions(n)
    return [i for i in range(pos % q, n, q) if i != pos and i not in zs]


def spread(n, d=D):
    """position -> value index for a batch of n: v(i) = (7 i + i // d) % d, which repeats at no fixed distance (v(i + d) =
    v(i) + 1; for a distance below d the difference is a non-zero constant, or that constant plus one); then the zero case
    at zero_positions(n), and a plain random value on every partner of a zero that the map gave a named case."""
    i = np.arange(n, dtype=np.int64)
    v = (7 * i + i // d) % d
    for z in zero_positions(n):
        v[z] = ZERO
        for p in partners(n, z):
            if v[p] < N_NAMED:
                v[p] = N_NAMED + (v[p] * 5 + p) % (d - N_NAMED)
    return v


DISTANCES = (1, 2, 3, 4, 16, 63, 64, 65, 128, 256)


def repeats(n, d=D):
    """{distance: positions i with v(i) == v(i + distance)} over the distances at which a kernel could read a neighbour's
    value: lanes, quads, waves, workgroups, the tile itself, the quarters of k_fe_inv4"""
    v = spread(n, d)
    q = (n + 3) // 4
    return {k: int(np.count_nonzero(v[:-k] == v[k:])) if k < n else 0 for k in DISTANCES + (d, q, 2 * q, 3 * q)}


def sizes(cus):
    """every batch size the GPU tests tile with spread() on a device of `cus` compute units"""
    tri_max, t = cus * 64, cus * 128
    return sorted({1, 63, 64, 65, 251, 2048, 2049, tri_max, tri_max + 1, t - 1, t, t + 1, t + 2, t + 3, 255, 256, 257, 1000})


def tile(rows, n, d=D, roll=0):
    """the batch of n: rows[spread(n)] joined, rows = d byte strings of one length; roll moves every value that many positions up
    (the last ones come round to the front), which takes the zeros off the positions spread() gives them"""
    a = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(d, -1)
    return a[np.roll(spread(n, d), roll)].tobytes()
