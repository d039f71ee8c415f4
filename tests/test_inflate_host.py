"""inflate.h (fp2_sqrt2, g1_inflate, g2_inflate) compiled for the host with -DBN_CHECK, so that every multiply asserts the
lazy-limb interval discipline: the square root against Python integers, the element functions against the oracle's
decompression byte for byte, and the counted cost of g2_inflate against g2_decompress.  A test tool; the product has no CPU
path."""
import ctypes
import random

import pytest

from tests import compressed_cases as cc
from tests import hostsim_build

P = cc.P


@pytest.fixture(scope="module")
def hs():
    so = hostsim_build.build("inflate_host.cpp", "libinflate.so")
    return ctypes.CDLL(so)


def mads(c):
    """the weights of tests/test_unit_pairs.py: multiply-adds per counted operation"""
    mul, sqr, dot, _norm, _lcs, terms = c
    return 162 * mul + 126 * sqr + 243 * dot + 9 * terms


def sqrt2(hs, a):
    out = ctypes.create_string_buffer(64)
    sq = hs.hs_inf_fp2_sqrt2(cc.be(a[0]) + cc.be(a[1]), out)
    assert sq in (0, 1)
    return sq, (int.from_bytes(out.raw[:32], "big"), int.from_bytes(out.raw[32:], "big"))


def f2_sqr(r):
    return ((r[0] * r[0] - r[1] * r[1]) % P, 2 * r[0] * r[1] % P)


def is_residue(v):
    return v % P == 0 or pow(v, (P - 1) // 2, P) == 1


def fp2_inputs():
    """(class, a): every class the method treats differently, decided with Python integers"""
    rnd = random.Random(17)
    qr = [v for v in (rnd.randrange(1, P) for _ in range(40)) if is_residue(v)][:6]
    nr = [v for v in (rnd.randrange(1, P) for _ in range(40)) if not is_residue(v)][:6]
    out = []
    for _ in range(12):
        out.append(("square", f2_sqr((rnd.randrange(P), rnd.randrange(P)))))
    while sum(1 for k, _ in out if k == "non-square") < 12:
        a = (rnd.randrange(P), rnd.randrange(P))
        if not is_residue(a[0] * a[0] + a[1] * a[1]):
            out.append(("non-square", a))
    out += [("a1 == 0, a0 a residue", (v, 0)) for v in qr]
    out += [("a1 == 0, a0 a non-residue", (v, 0)) for v in nr]           # a0 + s == 0: d == 0 on the first try, the (-h, x0) branch with h == 0
    out += [("a0 == 0", (0, v)) for v in qr[:3] + nr[:3]]
    out += [("a == 0", (0, 0)), ("1", (1, 0)), ("-1", (P - 1, 0)), ("u", (0, 1)), ("-u", (0, P - 1))]
    # d == 0 with a1 == 0 exactly: a0 = -s for the root s the chain gives of a0^2, i.e. a0 = -(v^2) for any v
    out += [("d == 0", ((-v * v) % P, 0)) for v in (2, 3, rnd.randrange(1, P))]
    return out


def test_fp2_sqrt2_against_python_integers(hs):
    seen = set()
    for kind, a in fp2_inputs():
        square = is_residue(a[0] * a[0] + a[1] * a[1])            # an element of Fp2 is a square iff its norm is one in Fp
        sq, r = sqrt2(hs, a)
        assert sq == (1 if square else 0), (kind, a)
        if square:
            assert f2_sqr(r) == a, (kind, a, r)
        seen.add((kind, sq))
    assert ("non-square", 0) in seen and ("square", 1) in seen and ("a1 == 0, a0 a non-residue", 1) in seen and ("d == 0", 1) in seen


def inflate(fn, c, width):
    out = ctypes.create_string_buffer(width)
    counts = (ctypes.c_double * 6)()
    ok = fn(c, out, counts)
    return out.raw, ok, [int(v) for v in counts]


def test_g1_inflate_equals_the_oracle_or_the_marker(hs, oracle):
    classes = cc.g1_classes(oracle)
    flags = set()
    for name, members in classes.items():
        for c in members:
            exp, st = cc.g1_expect(oracle, c)
            assert st == (1 if name in ("point", "identity") else 0), (name, c.hex())
            got, ok, _ = inflate(hs.hs_inf_g1, c, 64)
            assert (got, ok) == (exp, st), (name, c.hex())
            if name == "point":
                flags.add(c[0] >> 7)
                dec, dok, _ = inflate(hs.hs_inf_g1_decompress, c, 64)
                assert dok == 1 and dec == got
    assert flags == {0, 1}


def test_g2_inflate_equals_the_oracle_or_the_marker(hs, oracle):
    classes = cc.g2_classes(oracle)
    flags = set()
    for name, members in classes.items():
        for c in members:
            exp, st = cc.g2_expect(oracle, c)
            assert st == (1 if name in ("point", "identity") else 0), (name, c.hex())
            got, ok, _ = inflate(hs.hs_inf_g2, c, 128)
            assert (got, ok) == (exp, st), (name, c.hex())
            if name == "point":
                flags.add(c[0] >> 7)
    assert flags == {0, 1}
    for c in classes["point"][:4]:
        dec, dok, _ = inflate(hs.hs_inf_g2_decompress, c, 128)
        assert dok == 1 and dec == inflate(hs.hs_inf_g2, c, 128)[0]


def test_g2_inflate_costs_less_than_a_third_of_g2_decompress(hs, oracle):
    """Counted, not measured: the Fp operation counters of the BN_CHECK build on the same input, weighted by their multiply-adds.
    Two fixed chains of 251 squarings + 52 products against two 256-step square-and-always-multiply ladders in Fp2: about 0.24."""
    c = cc.g2_points(oracle, 2)[0]
    _, ok_i, ci = inflate(hs.hs_inf_g2, c, 128)
    _, ok_d, cd = inflate(hs.hs_inf_g2_decompress, c, 128)
    assert ok_i == 1 and ok_d == 1
    print("g2_inflate: %d multiply-adds %s; g2_decompress: %d %s; ratio %.3f" % (mads(ci), ci, mads(cd), cd, mads(ci) / mads(cd)))
    assert 3 * mads(ci) < mads(cd)
    # data-independent: a different input, an identity and an undecodable one run the same operations
    for other in (cc.g2_points(oracle, 4)[3], bytes(64), cc.be(P) + cc.be(1)):
        assert inflate(hs.hs_inf_g2, other, 128)[2] == ci
