"""CPU-only: one step of the prepared-key Miller loop, ell_pair_unit (pairing.h), which multiplies f by a unit line pair with
twelve Fp2 products (three 3 x 2 products over Fp2[w], each by evaluation at 0, inf, 1, -1) and returns TWICE f l.  Compiled for the
host with -DBN_CHECK (every multiply asserts the lazy-limb interval discipline) and compared coefficient by coefficient with the
Fp12 arithmetic of oracle/pyref: this pins the factor 2, which no test after the final exponentiation can see.  Operands are random
field elements, and limb patterns at the ends of the intervals the checker carries where the loop runs.  Operation counts of the
step and of the whole loop.  A test tool; the product has no CPU path."""
import ctypes
import math
import random
from fractions import Fraction

import pytest

from tests import hostsim_build

NL, RB = 9, 29
L = 1 << RB
RBITS = 261                                  # Montgomery R = 2^261
PARENT_LOOP_MADS = 1300536                   # the sixteen-product step (profiles/unit_pairs.json)
PARENT_STEP_DOTS = 40                        # 8 for the four coefficients + 2 x 16 Fp2 products
LOOP_MADS = 1132632                          # measured here: 88 x (32 double products + 52 fp_lc terms) + 65 squarings of f
ENTRY_TRK = (-4e-6, 1.0 + 4e-6, -0.02, 0.02, 1.2)      # the declared range of a pair-table entry (fp2_load_limbs_lazy)


@pytest.fixture(scope="module")
def hs():
    so = hostsim_build.build("pair_product_host.cpp", "libpairproduct.so")
    return ctypes.CDLL(so)


def limbs_of(m):
    """strict limbs of 0 <= m < 2^261"""
    return [(m >> (RB * i)) & (L - 1) for i in range(NL - 1)] + [m >> (RB * (NL - 1))]


def value_of(limbs, P):
    """the field element a limb vector stands for (Montgomery form, signed limbs)"""
    return sum(l << (RB * i) for i, l in enumerate(limbs)) * pow(1 << RBITS, -1, P) % P


def mont(x, P):
    return limbs_of(x * (1 << RBITS) % P)


def edge(trk, P, high, flip=False):
    """Limbs at one end of the interval (lo, hi, tlo, thi, vb): limbs 0..7 at hi (or lo; alternating from limb to limb with `flip`),
    the top limb as far out as its own interval and the value bound vb p allow."""
    lo, hi, tlo, thi, vb = trk
    low = [(math.floor(hi * L) if (high ^ (flip and i % 2 == 1)) else math.ceil(lo * L)) for i in range(NL - 1)]
    s = sum(l << (RB * i) for i, l in enumerate(low))
    bound = math.floor(Fraction(vb) * P)
    if high:
        top = min(math.floor(thi * L), (bound - s) >> (RB * (NL - 1)))
    else:
        top = max(math.ceil(tlo * L), -((bound + s) >> (RB * (NL - 1))))
    assert abs(s + (top << (RB * (NL - 1)))) <= bound and tlo * L <= top <= thi * L
    return low + [top]


def arr(limbs):
    flat = [l for v in limbs for l in v]
    return (ctypes.c_int32 * len(flat))(*flat)


def dbl(t):
    return (ctypes.c_double * 5)(*t)


def step(hs, pyref, f, ftrk, entry, cw, cwtrk, unit):
    """runs ell_pair_unit on limb vectors (f: 12, entry: 18, cw: 8) and returns (got, want, counts): the six w-coefficients"""
    P = pyref.P
    out = ctypes.create_string_buffer(384)
    counts = (ctypes.c_double * 6)()
    assert hs.hs_pp_step(arr(f), dbl(ftrk), arr(entry), arr(cw), dbl(cwtrk), 1 if unit else 0, out, counts) == 0
    got = [None] * 6
    fw = [None] * 6
    for k, wi in enumerate(pyref.TOWER_ORDER):
        got[wi] = (int.from_bytes(out.raw[64 * k:64 * k + 32], "big"), int.from_bytes(out.raw[64 * k + 32:64 * k + 64], "big"))
        fw[wi] = (value_of(f[2 * k], P), value_of(f[2 * k + 1], P))
    T = [(value_of(entry[2 * j], P), value_of(entry[2 * j + 1], P)) for j in range(9)]
    Y, Z, ysY, xsZ, ysZ, ysX, xsY, X = (value_of(c, P) for c in cw)
    dot = lambda t, s, u, r: pyref.f2_add(pyref.f2_muls(t, s), pyref.f2_muls(u, r))
    lw = [dot(T[0], ysY, T[1], Z), dot(T[5], ysX, T[6], xsY), (1 if unit else 0, 0), dot(T[7], ysZ, T[8], Y), dot(T[3], xsZ, T[4], X), (0, 0)]
    want = [pyref.f2_muls(c, 2) for c in pyref.f12_mul(fw, lw)]
    return got, want, [int(c) for c in counts]


def bounds(hs, pyref):
    rnd = random.Random(7)
    P = pyref.P
    entry = [mont(rnd.randrange(P), P) for _ in range(18)]
    xy = [mont(rnd.randrange(1, P), P) for _ in range(5)]
    out = (ctypes.c_double * 15)()
    assert hs.hs_pp_bounds(arr(entry), arr(xy), out) == 0
    b = [tuple(out[5 * k:5 * k + 5]) for k in range(3)]
    print("intervals (lo, hi, tlo, thi, vb): f after fp12_sqr %s, f after a pair step %s, coordinate value %s" % tuple(b))
    return b


def test_random_operands_give_twice_f_times_the_pair(hs, pyref):
    P = pyref.P
    rnd = random.Random(2024)
    f_sqr, _, cw_trk = bounds(hs, pyref)
    for trial in range(24):
        f = [mont(rnd.randrange(P), P) for _ in range(12)]
        entry = [mont(rnd.randrange(P), P) for _ in range(18)]
        cw = [mont(rnd.randrange(P), P) for _ in range(8)]
        unit = trial % 4 != 3
        got, want, _ = step(hs, pyref, f, f_sqr, entry, cw, cw_trk, unit)
        for k in range(6):
            assert got[k] == want[k], (trial, unit, k)


def test_operands_at_the_ends_of_their_intervals(hs, pyref):
    """f with the limbs fp12_sqr and a preceding pair step may leave, table entries at the ends of their declared range, coordinate
    values at the ends of a product's range; all high, all low, and mixed so that the differences the step forms are extreme too."""
    P = pyref.P
    f_sqr, f_pair, cw_trk = bounds(hs, pyref)
    for ftrk in (f_sqr, f_pair):
        for pattern in range(8):
            # bit 0: f high / low; bit 1: entry and coordinate values high / low; bit 2: alternate within the operand
            fh, eh, alt = bool(pattern & 1), bool(pattern & 2), bool(pattern & 4)
            f = [edge(ftrk, P, fh ^ (alt and (k // 2) % 2 == 1), flip=alt and k % 2 == 1) for k in range(12)]
            entry = [edge(ENTRY_TRK, P, eh ^ (alt and (j // 2) % 2 == 1), flip=alt and j % 2 == 0) for j in range(18)]
            cw = [edge(cw_trk, P, eh ^ (alt and j % 2 == 1)) for j in range(8)]
            for unit in (True, False):
                got, want, _ = step(hs, pyref, f, ftrk, entry, cw, cw_trk, unit)
                for k in range(6):
                    assert got[k] == want[k], (ftrk, pattern, unit, k)


def mads(c):
    mul, sqr, dot, _norm, _lcs, terms = c
    return 162 * mul + 126 * sqr + 243 * dot + 9 * terms


def test_operation_counts(hs, pyref):
    """One pair step: eight double products fewer than the sixteen-product form (40 -> 32), no single products.  The whole loop:
    fewer executed MADs than the parent's 1 300 536, at most the count measured when this form was written."""
    P = pyref.P
    rnd = random.Random(5)
    f_sqr, _, cw_trk = bounds(hs, pyref)
    f = [mont(rnd.randrange(P), P) for _ in range(12)]
    entry = [mont(rnd.randrange(P), P) for _ in range(18)]
    cw = [mont(rnd.randrange(P), P) for _ in range(8)]
    for unit in (True, False):
        _, _, c = step(hs, pyref, f, f_sqr, entry, cw, cw_trk, unit)
        print("pair step (unit = %s): mul, sqr, dot, norm, lc passes, lc terms = %s: %d MADs" % (unit, c, mads(c)))
        assert c[0] == 0 and c[1] == 0
        assert c[2] == PARENT_STEP_DOTS - 8
    table = [mont(rnd.randrange(P), P) for _ in range(88 * 18)]
    counts = (ctypes.c_double * 6)()
    assert hs.hs_pp_loop_counts(arr(table), arr(cw), dbl(cw_trk), 1, counts) == 0
    c = [int(x) for x in counts]
    print("loop: mul, sqr, dot, norm, lc passes, lc terms = %s: %d executed MADs (parent %d)" % (c, mads(c), PARENT_LOOP_MADS))
    assert c[2] == 88 * (PARENT_STEP_DOTS - 8) + 65 * 24
    assert mads(c) < PARENT_LOOP_MADS
    assert mads(c) <= LOOP_MADS
