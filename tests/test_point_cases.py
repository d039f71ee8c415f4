"""CPU-only: the edge-case and off-curve operands of tests/point_cases.py.  Every case is in the class it is filed under, by the
pure-Python model and by the oracle's checks; the oracle's pairing equals the independent affine-line model on named on-curve
pairs, points of the twist outside the r-torsion included; the device headers compiled for the host (the lane, wave-per-pair
and quad Miller loops, the quad key preparation and the prepared-key loop) give the oracle's Miller bytes on every named pair;
the tiling has no period and the verify table holds every kind of wrong tuple."""
import ctypes

import pytest

from tests import hostsim_build
from tests import point_cases as C
from tests.helpers import bits_of


@pytest.fixture(scope="module")
def hs():
    return ctypes.CDLL(hostsim_build.build("hostsim.cpp", "libhostsim.so"))


def test_every_case_is_in_its_class(oracle, pyref):
    P = pyref.P
    a, b = C.g1_cases(oracle, pyref), C.g2_cases(oracle, pyref)
    assert list(a.items()) == list(C._g1_build(pyref)[0].items()) and list(b.items()) == list(C._g2_build(pyref).items())     # repeatable
    assert len(set(v for _, v in a.values())) == len(a) and len(set(v for _, v in b.values())) == len(b)
    vals = [v for _, v in a.values()]
    assert C._g1(1, 2) in vals and C._g1(1, P - 2) in vals                    # the generator and its negative, under an edge name
    assert set(C.g1_aliases(oracle, pyref)) == {"gen", "neg_gen", "(r-1)G"}
    ys = [int.from_bytes(v[32:], "big") & 1 for name, (_, v) in a.items() if name.startswith("edge_")]
    assert 0 in ys and 1 in ys
    g1_ok = bits_of(oracle.g1_check_batch(b"".join(vals), len(a)), len(a))
    for (name, (cls, v)), ok in zip(a.items(), g1_ok):
        decodes, pt = pyref.g1_from_bytes(v)
        assert decodes, name                                                  # every coordinate below p: the raw calls take it
        assert (pt is None) == (cls == "identity"), name
        assert pyref.g1_on_curve(pt) == (cls != "off_curve"), name
        assert ok == (cls != "off_curve"), name                               # the oracle: on the curve, the identity included
    g2_ok = bits_of(oracle.g2_check_batch(b"".join(v for _, v in b.values()), len(b)), len(b))
    for (name, (cls, v)), ok in zip(b.items(), g2_ok):
        decodes, pt = pyref.g2_from_bytes(v)
        assert decodes, name
        assert (pt is None) == (cls == "identity"), name
        assert pyref.g2_on_curve(pt) == (cls != "off_curve"), name
        if cls in ("subgroup", "outside"):
            assert pyref.g2_in_subgroup_slow(pt) == (cls == "subgroup"), name
        assert ok == (cls in ("subgroup", "identity")), name
    for cls in C.G1_CLASSES:
        assert C.of_class(a, cls), cls
    for cls in C.G2_CLASSES:
        assert C.of_class(b, cls), cls
    assert len(C.of_class(b, "subgroup")) == 8 and len(C.of_class(b, "outside")) == 8
    for k, e in enumerate(C.mont_edge_values(P)):                             # the device's form of x is the edge value, a few units up
        assert (int.from_bytes(a["mont_%d" % k][1][:32], "big") * (1 << 261) - e) % P < 256, k


def test_pairs_cover_every_class_and_every_named_point(oracle, pyref):
    a, b = C.g1_cases(oracle, pyref), C.g2_cases(oracle, pyref)
    names, g1s, g2s, mls, gts = C.pairs(oracle, pyref)
    k = C.n_named(oracle, pyref)
    assert len(names) == len(set(zip(g1s, g2s))) == C.D and all(n is not None for n in names[:k]) and names[k:] == [None] * (C.D - k)
    assert {(a[x][0], b[y][0]) for x, y in names[:k]} == {(ca, cb) for ca in C.G1_CLASSES for cb in C.G2_CLASSES}
    assert {x for x, _ in names[:k]} == set(a) and {y for _, y in names[:k]} == set(b)
    for i in range(C.D):
        g1_ident = names[i] is not None and a[names[i][0]][0] == "identity"
        g2_ident = names[i] is not None and b[names[i][1]][0] == "identity"
        assert (mls[i] == C.ONE_GT) == (g1_ident or g2_ident), names[i]       # identity by encoding: the Miller value is one
        if i >= k:
            assert gts[i] != C.ONE_GT


# the named pairs of the comparison with the affine-line model: on-curve points only (its lines are not defined elsewhere).  A pair
# on which a line's denominator vanishes (T = +-Q within the loop: the slope's inverse of zero) would be left out HERE and
# nowhere else, by name; none of the pairs below does.
PYREF_LEFT_OUT = ()


def test_oracle_pairing_equals_affine_line_model(oracle, pyref):
    """the reference itself on edge-case points: the C oracle (projective lines, sparse products) against the pure-Python model
    (affine lines, dense Fp12) on 12 named pairs with a G2 member of the subgroup and 12 with one outside the r-torsion"""
    a, b = C.g1_cases(oracle, pyref), C.g2_cases(oracle, pyref)
    names, g1s, g2s, mls, gts = C.pairs(oracle, pyref)
    picked = {"subgroup": [], "outside": []}
    for i, n in enumerate(names):
        if n is not None and a[n[0]][0] == "curve" and b[n[1]][0] in picked and n not in PYREF_LEFT_OUT and len(picked[b[n[1]][0]]) < 12:
            picked[b[n[1]][0]].append(i)
    assert len(picked["subgroup"]) == 12 and len(picked["outside"]) == 12
    for i in picked["subgroup"] + picked["outside"]:
        pt, q = pyref.g1_from_bytes(g1s[i])[1], pyref.g2_from_bytes(g2s[i])[1]
        assert pyref.f12_to_bytes(pyref.pairing(pt, q)) == gts[i], names[i]


def test_host_miller_forms_equal_oracle_on_named_pairs(hs, oracle, pyref):
    """lane_miller_1 (k_miller_1), wide_miller_1 (k_miller_wide_1) and tri_miller_1 (k_miller_tri_1) on the host under the
    interval checker, on every named pair: the oracle's Miller bytes.  A pair with an identity member goes through lane_miller_1
    alone: the helpers of the other two forms refuse it or leave the skip to the kernel."""
    a, b = C.g1_cases(oracle, pyref), C.g2_cases(oracle, pyref)
    names, g1s, g2s, mls, gts = C.pairs(oracle, pyref)
    out = ctypes.create_string_buffer(768); out2 = ctypes.create_string_buffer(384); st = ctypes.c_int(0)
    for i in range(C.n_named(oracle, pyref)):
        ident = "identity" in (a[names[i][0]][0], b[names[i][1]][0])
        hs.hs_miller1(g1s[i], g2s[i], out, ctypes.byref(st))
        assert out.raw[:384] == mls[i] and st.value & 3 == 3, names[i]
        if ident:
            assert hs.hs_tri_miller_1(g1s[i], g2s[i], out, out2) == -1, names[i]
            continue
        assert hs.hs_miller_wide_var(g1s[i], g2s[i], out) == 0 and out.raw[:384] == out.raw[384:] == mls[i], names[i]
        assert hs.hs_tri_miller_1(g1s[i], g2s[i], out, out2) == 0 and out.raw[:384] == out2.raw == mls[i], names[i]


def test_host_prepared_forms_equal_oracle_on_subgroup_keys(hs, oracle, pyref):
    """quad_prepare_lines / quad_torsion_free (k_g2_prepare_quad) against the one-lane preparation, and tri_miller_1prepared over
    the key's table, for every G1 case against every key of the subgroup"""
    a, b = C.g1_cases(oracle, pyref), C.g2_cases(oracle, pyref)
    bits = ctypes.c_int(0)
    out = ctypes.create_string_buffer(384); out2 = ctypes.create_string_buffer(384)
    for name in C.of_class(b, "subgroup") + C.of_class(b, "outside"):
        assert hs.hs_quad_prepare(b[name][1], ctypes.byref(bits)) == 1, name         # the quad's table is the serial one, limb for limb
        assert bits.value == (7 if b[name][0] == "subgroup" else 4), name           # both say "in" / both say "outside", all lanes agree
    for q in C.of_class(b, "subgroup"):
        want = oracle.miller_loop_batch(b"".join(v for _, v in a.values()), b[q][1] * len(a), len(a))
        for k, (p, (cls, v)) in enumerate(a.items()):
            if cls == "identity":
                assert hs.hs_tri_miller_1prepared(v, b[q][1], out, out2) == -1 and want[384 * k:384 * k + 384] == C.ONE_GT, (p, q)
                continue
            assert hs.hs_tri_miller_1prepared(v, b[q][1], out, out2) == 0 and out.raw == out2.raw == want[384 * k:384 * k + 384], (p, q)


@pytest.mark.parametrize("cus", [256, 128, 64, 32])
def test_spread_has_no_period(cus):
    for n in C.sizes(cus):
        v = C.spread(n)
        assert len(v) == n and v.min() >= 0 and v.max() < C.D
        for dist, count in C.repeats(n).items():
            assert count < 0.02 * n, (n, dist, count)
        if n >= C.D:
            assert len(set(v.tolist())) == C.D                                # every pair is in the batch
    rows = [bytes([i]) * 3 for i in range(C.D)]
    assert C.tile(rows, 300) == b"".join(rows[i] for i in C.spread(300))


def test_verify_table_holds_every_kind(oracle, pyref):
    kinds, pks, msgs, sigs, bits = C.verify_table(oracle, pyref, pyref.DEFAULT_DST)
    assert len(kinds) == len(set(zip(pks, msgs, sigs))) == C.D and len(set(msgs)) == C.D
    assert sum(bits) >= 0.4 * C.D
    for kind, bit in zip(kinds, bits):
        assert bit == (kind == "honest"), kind
    assert set(kinds) == {"honest"} | set(C.INVALID_KINDS)
    a = C.g1_cases(oracle, pyref)
    assert {v for _, v in a.values()} <= set(sigs)                            # every named G1 case stands as a "signature"
    assert all(pks.count(pk) >= 2 for pk in set(pks))                         # no key with one tuple
    neg_g2 = pyref.g2_to_bytes(pyref.g2_neg(pyref.G2_GEN))
    assert any(pk == neg_g2 and bit for pk, bit in zip(pks, bits))            # the check's own second key as a public key
    for n in (65, 300):                                                       # a small batch holds valid and invalid tuples
        got = [bits[v] for v in C.spread(n)]
        assert True in got and False in got


def test_check_groups_are_what_they_claim(oracle, pyref):
    """{(P, Q), (-P, Q)}: the oracle's product of pairings is one for Q on the twist, inside the r-torsion or not"""
    groups = C.check_groups(oracle, pyref)
    assert {want for _, _, _, want in groups} == {True, False}
    for label, g1, g2, want in groups:
        one = oracle.final_exponentiation(oracle.multi_miller_loop(g1, g2, 2), 1) == C.ONE_GT
        if want or "outside" in label:
            assert one, label
