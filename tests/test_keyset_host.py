"""CPU-only: proj_add_mixed (bls-bn254_amd/csrc/curve.h) and the lane functions of the sums over a registered key set
(bls-bn254_amd/csrc/keyset.h) compiled for the host with -DBN_CHECK, so the interval bounds of the mixed addition are checked
on every call: the mixed addition against the full one and against the pure-Python G2 arithmetic, and the whole pipeline --
registration, flip / ok, the per-word masks, the word sums, the reduction passes over word-major partials, the complement --
against a Python model for key sets that cross word and pass boundaries.  A test tool; the product has no CPU path."""
import ctypes
import random

import pytest

from tests import hostsim_build
from tests import synth
from tests.helpers import IDENT2, row_of

N_KEYS = [1, 31, 32, 33, 70, 513]           # 513: W = 17 words, two reduction passes


@pytest.fixture(scope="module")
def hs():
    so = hostsim_build.build("keyset_host.cpp", "libkeysethost.so")
    return ctypes.CDLL(so)


def add_mixed(hs, a, p_identity, q):
    om, of = ctypes.create_string_buffer(128), ctypes.create_string_buffer(128)
    assert hs.hs_ks_add_mixed(a, int(p_identity), q, om, of) == 1
    return om.raw, of.raw


def test_mixed_addition_equals_the_full_one(hs, pyref):
    B = pyref
    rnd = random.Random(5)
    enc = B.g2_to_bytes
    pts = [B.g2_mul(B.G2_GEN, rnd.randrange(1, B.R)) for _ in range(4)]
    out = B.g2_from_bytes(synth.NON_SUBGROUP_PK)[1]
    assert B.g2_on_curve(out) and not B.g2_in_subgroup_fast(out)
    cases = []                                                        # (A, P is the identity, Q, P + Q)
    for a in pts[:3]:
        for q in pts[1:]:
            cases.append((a, False, q, B.g2_add(B.g2_add(a, a), q)))                       # random P and Q
    cases.append((pts[0], True, pts[1], pts[1]))                                          # P = identity
    cases.append((pts[0], False, B.g2_add(pts[0], pts[0]), B.g2_mul(pts[0], 4)))          # P = Q: doubling through the addition
    cases.append((pts[0], False, B.g2_neg(B.g2_add(pts[0], pts[0])), None))               # P = -Q
    cases.append((pts[2], False, out, B.g2_add(B.g2_add(pts[2], pts[2]), out)))            # Q outside the r-torsion
    cases.append((out, False, out, B.g2_add(B.g2_add(out, out), out)))                    # ... and P too
    cases.append((out, False, B.g2_add(out, out), B.g2_add(B.g2_add(out, out), B.g2_add(out, out))))
    cases.append((out, False, B.g2_neg(B.g2_add(out, out)), None))
    cases.append((out, True, out, out))
    for a, ident, q, want in cases:
        mixed, full = add_mixed(hs, enc(a), ident, enc(q))
        assert mixed == full == enc(want)


def key_set(B, n, rnd):
    """n encodings and their kinds: random keys with, where the set is large enough, an identity key, an off-curve key, an
    undecodable key, P and -P, and one key at two indices"""
    pts = [B.g2_mul(B.G2_GEN, rnd.randrange(1, B.R)) for _ in range(min(n, 12))]
    keys = [B.g2_to_bytes(pts[i % len(pts)] if i < 12 else B.g2_add(pts[i % 12], pts[(i // 12) % 12])) for i in range(n)]
    bad, ident = set(), set()
    if n >= 31:
        where = {"ident": 3, "off": 5, "undec": n - 2, "p": 7, "negp": n // 2, "dup_a": 1, "dup_b": n - 1}
        keys[where["ident"]] = IDENT2; ident.add(where["ident"])
        off = bytearray(keys[where["off"]]); off[127] ^= 1
        keys[where["off"]] = bytes(off); bad.add(where["off"])
        keys[where["undec"]] = b"\xff" * 32 + keys[where["undec"]][32:]; bad.add(where["undec"])
        keys[where["negp"]] = B.g2_to_bytes(B.g2_neg(B.g2_from_bytes(keys[where["p"]])[1]))
        keys[where["dup_b"]] = keys[where["dup_a"]]
    return keys, bad, ident


def rows_for(n, rnd, bad):
    """the patterns of the issue; every row is a set of key indices"""
    rows = [set(), set(range(n)), {n - 1}]
    for w in range((n + 31) // 32):
        rows.append({32 * w}); rows.append({min(32 * w + 31, n - 1)})
    rows = rows[:11]
    good = [i for i in range(n) if i not in bad]
    rows.append(set(rnd.sample(range(n), n // 2)))                    # exactly n/2 bits: not flipped
    rows.append(set(rnd.sample(range(n), min(n, n // 2 + 1))))        # n/2 + 1: the flip boundary
    rows.append(set(rnd.sample(good, min(len(good), n // 2 + 1))))    # flipped, the bad keys left unselected
    rows.append(set(range(n)) - bad)
    for dens in (0.1, 0.5, 0.9):
        rows.append({i for i in range(n) if rnd.random() < dens})
    return rows


@pytest.mark.parametrize("n", N_KEYS)
def test_pipeline_against_the_model(hs, pyref, n):
    B = pyref
    rnd = random.Random(1000 + n)
    keys, bad, ident = key_set(B, n, rnd)
    rows = rows_for(n, rnd, bad)
    G, W = len(rows), (n + 31) // 32
    sel = b"".join(row_of(r, n) for r in rows)
    bad_w, skip_w = (ctypes.c_uint32 * W)(), (ctypes.c_uint32 * W)()
    flip, ok = ctypes.create_string_buffer(G), ctypes.create_string_buffer(G)
    masks = (ctypes.c_uint32 * (W * G))()
    out = ctypes.create_string_buffer(128 * G)
    passes = hs.hs_ks_run(b"".join(keys), n, sel, G, bad_w, skip_w, flip, ok, masks, out)
    assert passes == (1 if W <= 16 else 2)
    skip = bad | ident
    assert {32 * w + b for w in range(W) for b in range(32) if (bad_w[w] >> b) & 1} == bad
    assert {32 * w + b for w in range(W) for b in range(32) if (skip_w[w] >> b) & 1} == skip
    pts = [None if i in skip else B.g2_from_bytes(keys[i])[1] for i in range(n)]
    for g, r in enumerate(rows):
        want_flip = 2 * len(r) > n
        want_ok = not (r & bad)
        assert (flip.raw[g], ok.raw[g]) == (int(want_flip), int(want_ok)), (n, g)
        added = (set(range(n)) - r if want_flip else r) - skip
        assert {32 * w + b for w in range(W) for b in range(32) if (masks[w * G + g] >> b) & 1} == added, (n, g)
        acc = None
        if want_ok:
            for i in sorted(r - skip):
                acc = B.g2_add(acc, pts[i])
        assert out.raw[128 * g:128 * g + 128] == B.g2_to_bytes(acc), (n, g, sorted(r)[:8])
