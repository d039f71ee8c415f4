"""Edge-case and off-curve operands for the calls that only DECODE their points (pairing_batch, miller_loop_batch, multi_miller_loop,
multi_miller_loop_batch, multi_miller_loop_prepared) and for the verify path: named G1 and G2 cases by class, D distinct pairs with
the oracle's Miller and pairing values (computed once per run), D verify tuples with the oracle's bits, and the map that tiles
them over a batch without a period.  A support module in the shape of fp12_cases.py: the CPU test of the cases and the GPU test
of the Miller-loop forms import it."""
import random
from collections import OrderedDict

import numpy as np

from tests.helpers import EDGE_COEFFS, IDENT1, IDENT2, b32

D = 251                                   # distinct pairs (and verify tuples) per run: a prime, as in fp12_cases
ONE_GT = b32(1) + bytes(352)
G1_CLASSES = ("curve", "identity", "off_curve")
G2_CLASSES = ("subgroup", "outside", "identity", "off_curve")          # identity: x = (0, 0), whatever y is
_cache = {}


def known_sks(R):
    """the secret keys of the first five `subgroup` keys"""
    return (1, 2, 3, R - 1, R - 2)


def mont_rinv(P):
    """the device holds a coordinate x as x 2^261 mod p in nine limbs of 29 bits (fp29.h): e MONT_RINV has the limbs of e there"""
    return pow(1 << 261, -1, P)


def mont_edges(P):
    """coordinates whose device form is a limb-boundary value: a single low limb, a full low limb, one bit in limb 2, one bit
    in the top limb, eight full limbs, p - 1"""
    return tuple(e * mont_rinv(P) % P for e in mont_edge_values(P))


def mont_edge_values(P):
    return (1 << 29, (1 << 29) - 1, 1 << 58, 1 << 232, (1 << 232) - 1, P - 1)


def _g1(x, y):
    return b32(x) + b32(y)


def _g2(x, y):
    """x, y = (c0, c1); the encoding is x.c1 | x.c0 | y.c1 | y.c0"""
    return b32(x[1]) + b32(x[0]) + b32(y[1]) + b32(y[0])


def g1_cases(oracle, pyref):
    """name -> (class, 64 bytes), in a fixed order, all distinct.  A case whose bytes an earlier name already has is left out (the
    edge coefficients 0 and 1 both give x = 1, and [r - 1]G is (1, p - 2)): g1_aliases() says which name stands for it."""
    if "g1" not in _cache:
        _cache["g1"] = _g1_build(pyref)
    return _cache["g1"][0]


def g1_aliases(oracle, pyref):
    """left-out name -> the name that has its bytes"""
    g1_cases(oracle, pyref)
    return _cache["g1"][1]


def _g1_build(pyref):
    P, R = pyref.P, pyref.R
    c = OrderedDict()
    alias = {}

    def put(name, cls, b):
        for other, (_, ob) in c.items():
            if ob == b:
                alias[name] = other
                return
        c[name] = (cls, b)
    for k, e in enumerate(EDGE_COEFFS):                    # the smallest x >= e on the curve, both signs of y over the cases
        x = max(e, 1)
        while pyref.fp_sqrt((x * x * x + 3) % P) is None:
            x += 1
        y = pyref.fp_sqrt((x * x * x + 3) % P)
        put("edge_%d" % k, "curve", _g1(x, P - y if k & 1 else y))
    for k, x in enumerate(mont_edges(P)):                  # the same for the limbs the device holds, both signs again
        while x == 0 or pyref.fp_sqrt((x * x * x + 3) % P) is None:
            x = (x + mont_rinv(P)) % P                     # one up in limb 0 of the device's form
        y = pyref.fp_sqrt((x * x * x + 3) % P)
        put("mont_%d" % k, "curve", _g1(x, P - y if k & 1 else y))
    put("gen", "curve", _g1(1, 2))
    put("neg_gen", "curve", _g1(1, P - 2))
    for name, k in (("2G", 2), ("3G", 3), ("(r-1)G", R - 1)):
        put(name, "curve", pyref.g1_to_bytes(pyref.g1_mul(pyref.G1_GEN, k)))
    put("identity", "identity", IDENT1)
    put("identity_y5", "identity", _g1(0, 5))              # x = 0 decodes as the identity whatever y is
    rnd = random.Random(0x9a1)
    for name, (x, y) in (("off_1_1", (1, 1)), ("off_pm1", (P - 1, P - 1)), ("off_y0", (1, 0)), ("off_limbs", ((1 << 29) - 1, 1 << 232)),
                         ("off_rand_0", (rnd.randrange(1, P), rnd.randrange(P))), ("off_rand_1", (rnd.randrange(1, P), rnd.randrange(P)))):
        assert not pyref.g1_on_curve((x, y))
        put(name, "off_curve", _g1(x, y))
    return c, alias


def _twist_point(pyref, x):
    """the first point of the twist at or after x = (c0, c1), c0 bumped until x^3 + b' is a square"""
    while True:
        y = pyref.f2_sqrt(pyref.f2_add(pyref.f2_mul(pyref.f2_sqr(x), x), pyref.B2))
        if y is not None and x != (0, 0):
            return (x, y)
        x = ((x[0] + 1) % pyref.P, x[1])


def outside_x(P):
    """where the search for the `outside` points starts, as (c0, c1)"""
    return ((0, 1), (1, 0), (0, P - 1), (P - 1, P - 1), (1 << 29, (1 << 29) - 1), ((1 << 232) - 1, 1 << 253), (P // 3, 0))


def g2_cases(oracle, pyref):
    """name -> (class, 128 bytes), in a fixed order, all distinct"""
    if "g2" not in _cache:
        _cache["g2"] = _g2_build(pyref)
    return _cache["g2"]


def _g2_build(pyref):
    P, R = pyref.P, pyref.R
    c = OrderedDict()
    for k in known_sks(R):
        c["[%s]G2" % (k if k < 4 else "r-%d" % (R - k))] = ("subgroup", pyref.g2_to_bytes(pyref.g2_mul(pyref.G2_GEN, k)))
    outside = [_twist_point(pyref, x) for x in outside_x(P)]
    for k, pt in enumerate(outside[:3]):
        c["cleared_%d" % k] = ("subgroup", pyref.g2_to_bytes(pyref.g2_clear_cofactor(pt)))
    for k, pt in enumerate(outside):
        c["outside_%d" % k] = ("outside", pyref.g2_to_bytes(pt))
    m = mont_edges(P)                                      # ... and one whose halves are limb-boundary values in the device's form
    x = (m[0], m[4])
    while pyref.f2_sqrt(pyref.f2_add(pyref.f2_mul(pyref.f2_sqr(x), x), pyref.B2)) is None:
        x = ((x[0] + mont_rinv(P)) % P, x[1])
    c["outside_mont"] = ("outside", pyref.g2_to_bytes(_twist_point(pyref, x)))
    c["identity"] = ("identity", IDENT2)
    rnd = random.Random(0x9a2)
    c["identity_y"] = ("identity", _g2((0, 0), (rnd.randrange(P), rnd.randrange(P))))
    E = EDGE_COEFFS
    off = [("off_y0", (1, 0), (0, 0)), ("off_pm1", (P - 1, P - 1), (P - 1, P - 1)), ("off_units", (0, 1), (1, 0)),
           ("off_limbs_a", ((1 << 29) - 1, 1 << 29), (1 << 58, 1 << 232)), ("off_limbs_b", ((1 << 232) - 1, 1 << 253), ((1 << 253) - 1, P // 3)),
           ("off_halves", (P - 2, 2), ((P + 1) // 2, (P - 1) // 2)), ("off_x_c1_0", (3, 0), (0, 3)), ("off_x_c0_0", (0, 3), (P - 1, 0)),
           ("off_rand_0", (rnd.randrange(P), rnd.randrange(P)), (rnd.randrange(P), rnd.randrange(P))),
           ("off_rand_1", (rnd.randrange(P), rnd.randrange(P)), (rnd.randrange(P), rnd.randrange(P)))]
    for name, x, y in off:
        assert x != (0, 0) and not pyref.g2_on_curve((x, y)), name
        if not name.startswith("off_rand"):
            assert all(v in E for v in x + y), name
        c[name] = ("off_curve", _g2(x, y))
    assert len(set(b for _, b in c.values())) == len(c)
    return c


def of_class(cases, cls):
    return [name for name, (k, _) in cases.items() if k == cls]


def named_pairs(oracle, pyref):
    """[((G1 name, G2 name), 64 bytes, 128 bytes)]: every G1 class against every G2 class, the longer list of names once and the
    shorter one cycled, so every named point occurs in every class of partners"""
    a, b = g1_cases(oracle, pyref), g2_cases(oracle, pyref)
    out = []
    for ca in G1_CLASSES:
        for cb in G2_CLASSES:
            na, nb = of_class(a, ca), of_class(b, cb)
            o = len(out)                                   # another partner for a name each time its class comes round
            for k in range(max(len(na), len(nb))):
                x, y = na[k % len(na)], nb[(k + o) % len(nb)]
                out.append(((x, y), a[x][1], b[y][1]))
    return out


def pairs(oracle, pyref):
    """(names, g1s, g2s, mls, gts): the named pairs followed by seeded random valid pairs, D distinct pairs in all (names[i] is None
    for the random ones), and oracle.miller_loop_batch / oracle.pairing_batch of each pair.  Computed on the first call of a run;
    callers do not change them."""
    if "pairs" not in _cache:
        named = named_pairs(oracle, pyref)
        names, g1s, g2s = [n for n, _, _ in named], [p for _, p, _ in named], [q for _, _, q in named]
        assert len(named) < D
        rnd = random.Random(0x9a3)
        G1, G2 = oracle.g1_generator(), oracle.g2_generator()
        while len(names) < D:
            names.append(None)
            g1s.append(oracle.g1_mul(G1, rnd.randrange(1, pyref.R))); g2s.append(oracle.g2_mul(G2, rnd.randrange(1, pyref.R)))
        assert len(set(zip(g1s, g2s))) == D
        ml = oracle.miller_loop_batch(b"".join(g1s), b"".join(g2s), D)
        gt = oracle.pairing_batch(b"".join(g1s), b"".join(g2s), D)
        _cache["pairs"] = (names, g1s, g2s, [ml[384 * i:384 * i + 384] for i in range(D)], [gt[384 * i:384 * i + 384] for i in range(D)])
    return _cache["pairs"]


def n_named(oracle, pyref):
    """pairs()[:n_named] are the named pairs"""
    return sum(n is not None for n in pairs(oracle, pyref)[0])


INVALID_KINDS = ("g1_case", "identity_sig", "off_curve_sig", "outside_key", "off_curve_key", "identity_key")


def verify_table(oracle, pyref, dst):
    """(kinds, pks, msgs, sigs, bits): D verify tuples and oracle.verify_batch of them, once per run.  kinds[i] is "honest" for a
    signature by the key's secret key, else one of INVALID_KINDS.  Honest tuples cycle over the five keys of known secret key
    (r - 1 gives -G2gen, the constant second key of the check itself); every named G1 case stands as a "signature" under one of
    those keys; keys of class outside, off_curve and identity carry two tuples each, so that no key of the table has one tuple."""
    if ("verify", dst) not in _cache:
        R = pyref.R
        a, b = g1_cases(oracle, pyref), g2_cases(oracle, pyref)
        sks = known_sks(R)
        keys = [b[n][1] for n in of_class(b, "subgroup")[:len(sks)]]
        assert keys[0] == oracle.g2_generator() and all(keys[k] == oracle.sk_to_pk(s) for k, s in enumerate(sks))
        msg = lambda i: b"point cases, tuple %d" % i
        rows = []
        for k, (name, (cls, pt)) in enumerate(a.items()):
            kind = {"curve": "g1_case", "identity": "identity_sig", "off_curve": "off_curve_sig"}[cls]
            rows.append((kind, keys[k % len(keys)], pt))
        some_sig = a["2G"][1]
        for kind, name in (("outside_key", "outside_0"), ("outside_key", "outside_3"), ("off_curve_key", "off_y0"), ("off_curve_key", "off_limbs_a"),
                           ("identity_key", "identity")):
            rows += [(kind, b[name][1], some_sig), (kind, b[name][1], a["edge_2"][1])]
        n_bad = len(rows)
        kinds, pks, msgs, sigs = [], [], [], []
        # one wrong tuple after every third honest one until they are used up: a small batch holds both
        bad = iter(rows)
        for i in range(D):
            row = next(bad, None) if i % 4 == 3 else None
            m = msg(i)
            if row is None:
                k = i % len(sks)
                row = ("honest", keys[k], oracle.sign(sks[k], m, dst))
            kinds.append(row[0]); pks.append(row[1]); msgs.append(m); sigs.append(row[2])
        assert next(bad, None) is None and kinds.count("honest") == D - n_bad
        bm = oracle.verify_batch(b"".join(pks), msgs, b"".join(sigs), dst)
        _cache[("verify", dst)] = (kinds, pks, msgs, sigs, [bool(bm[i >> 3] >> (i & 7) & 1) for i in range(D)])
    return _cache[("verify", dst)]


def spread(n, d=D):
    """position -> index for a batch of n: v(i) = (7 i + i // d) % d, which repeats at no fixed distance (see fp12_cases.spread)"""
    i = np.arange(n, dtype=np.int64)
    return (7 * i + i // d) % d


DISTANCES = (1, 2, 3, 4, 16, 63, 64, 65, 128, 256)


def repeats(n, d=D):
    """{distance: positions i with v(i) == v(i + distance)} over the distances at which a kernel could read a neighbour's operands:
    lanes (the two pairs of a k_miller_hpk2p lane), quads, waves, workgroups, the tile itself"""
    v = spread(n, d)
    return {k: int(np.count_nonzero(v[:-k] == v[k:])) if k < n else 0 for k in DISTANCES + (d,)}


def sizes(cus):
    """every batch size the GPU tests tile with spread() on a device of `cus` compute units"""
    tri_max = cus * 64
    return sorted({1, 2, 3, 63, 64, 65, 251, 300, 1024, 1025, 2048, 2049, 2050, tri_max, tri_max + 1})


def tile(rows, n, d=D):
    """the batch of n: rows[spread(n)] joined, rows = d byte strings of one length"""
    a = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(d, -1)
    return a[spread(n, d)].tobytes()


def check_groups(oracle, pyref):
    """[(label, g1 bytes, g2 bytes, want bit)] for pairing_check_batch: groups {(P, Q), (-P, Q)}, whose product of pairings is 1
    wherever the pairing is defined.  set: P an edge G1 case, Q in the subgroup; cleared: Q on the twist outside the r-torsion
    (the product is still 1: the torsion test alone clears the bit), or either member off its curve."""
    P = pyref.P
    a, b = g1_cases(oracle, pyref), g2_cases(oracle, pyref)
    neg = lambda pt: pt[:32] + b32(-int.from_bytes(pt[32:], "big") % P)
    out = []
    edge = [n for n in of_class(a, "curve") if n.startswith("edge_")]
    for k, q in enumerate(of_class(b, "subgroup")):
        p = a[edge[k % len(edge)]][1]
        out.append(("%s x %s" % (edge[k % len(edge)], q), p + neg(p), b[q][1] * 2, True))
    for k, q in enumerate(of_class(b, "outside")):
        p = a[edge[(k + 5) % len(edge)]][1]
        out.append(("%s x %s" % (edge[(k + 5) % len(edge)], q), p + neg(p), b[q][1] * 2, False))
    for k, q in enumerate(of_class(b, "off_curve")[:4]):
        p = a[edge[k]][1]
        out.append(("%s x %s" % (edge[k], q), p + neg(p), b[q][1] * 2, False))
    for k, pn in enumerate(of_class(a, "off_curve")[:4]):
        q = of_class(b, "subgroup")[k]
        out.append(("%s x %s" % (pn, q), a[pn][1] + neg(a[pn][1]), b[q][1] * 2, False))
    return out
