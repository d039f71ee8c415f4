"""Compressed G1 / G2 encodings of every class the inflate stage has to tell apart, with what the oracle makes of them.
Shared by tests/test_inflate_host.py (the lane functions on the host) and tests/test_gpu_compressed.py (the kernels).
Test data generation only."""
import random

P = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
MARK1 = b"\xff" * 64
MARK2 = b"\xff" * 128


def be(v):
    return v.to_bytes(32, "big")


def flagged(c, flag):
    return bytes([(c[0] & 0x7f) | (flag << 7)]) + c[1:]


def g1_no_point(oracle, rnd, count):
    """x < p with x^3 + 3 a non-residue, found by drawing until the oracle does not decode"""
    out = []
    while len(out) < count:
        c = be(rnd.randrange(1, P))
        if oracle.g1_decompress(c) is None:
            out.append(c)
    return out


def g2_no_point(oracle, rnd, count):
    out = []
    while len(out) < count:
        c = be(rnd.randrange(P)) + be(rnd.randrange(P))
        if oracle.g2_decompress(c) is None:
            out.append(c)
    return out


def g1_points(oracle, count):
    """compressed k G and -(k G) for k = 1 .. count / 2: both flag values occur"""
    G = oracle.g1_generator()
    out = []
    for k in range(1, count // 2 + 1):
        c = oracle.g1_compress(oracle.g1_mul(G, 7 * k + 1))
        out += [c, flagged(c, 1 - (c[0] >> 7))]
    return out


def g2_points(oracle, count):
    G = oracle.g2_generator()
    out = []
    for k in range(1, count // 2 + 1):
        c = oracle.g2_compress(oracle.g2_mul(G, 5 * k + 2))
        out += [c, flagged(c, 1 - (c[0] >> 7))]
    return out


def g1_classes(oracle, points=40, seed=5):
    """{class name: [compressed encodings]}"""
    rnd = random.Random(seed)
    big = [be(P), be(P + 1), be((1 << 255) - 1)]
    return {
        "point": g1_points(oracle, points),
        "identity": [bytes(32), flagged(bytes(32), 1)],
        "x>=p": big + [flagged(c, 1) for c in big],
        "no point": [flagged(c, f) for c in g1_no_point(oracle, rnd, 6) for f in (0, 1)],
    }


def g2_classes(oracle, points=40, seed=6):
    rnd = random.Random(seed)
    big = [P, P + 1, (1 << 255) - 1]
    ok = rnd.randrange(P)
    return {
        "point": g2_points(oracle, points),
        "identity": [bytes(64), flagged(bytes(64), 1)],
        "x.c1>=p": [flagged(be(v) + be(ok), f) for v in big for f in (0, 1)],
        "x.c0>=p": [flagged(be(ok) + be(v), f) for v in big + [(1 << 256) - 1] for f in (0, 1)],
        "no point": [flagged(c, f) for c in g2_no_point(oracle, rnd, 6) for f in (0, 1)],
    }


def g1_expect(oracle, c):
    """(64 bytes, status) the inflate stage must give for one encoding: the oracle's bytes, or the marker"""
    r = oracle.g1_decompress(c)
    return (r, 1) if r is not None else (MARK1, 0)


def g2_expect(oracle, c):
    r = oracle.g2_decompress(c)
    return (r, 1) if r is not None else (MARK2, 0)


def mixed(classes, n, seed):
    """n encodings cycling through the classes' members in a seeded order (every member appears when n allows; points repeat)"""
    pool = [c for name in sorted(classes) for c in classes[name]]
    rnd = random.Random(seed)
    out = list(pool)
    while len(out) < n:
        out.append(pool[rnd.randrange(len(pool))])
    rnd.shuffle(out)
    return out[:n] if n < len(pool) else out
