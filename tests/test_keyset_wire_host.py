"""CPU-only: the lane functions behind the wire-format forms of the checked aggregation calls (g1_inflate_point of inflate.h,
ka_scan_wire / ka_wire_out of keyset_agg.h, kca_scan_wire of keyset_committee_agg.h) compiled for the host with -DBN_CHECK, each
against the function it has to agree with: g1_inflate, ka_scan / kca_scan on the inflated bytes, the oracle's g1_compress.  A
test tool; the product has no CPU path."""
import ctypes

import numpy as np
import pytest

from tests import compressed_cases as cc
from tests import hostsim_build
from tests.helpers import bitmap, IDENT1

u32p = ctypes.POINTER(ctypes.c_uint32)


@pytest.fixture(scope="module")
def hs():
    so = hostsim_build.build("keyset_wire_host.cpp", "libkeysetwirehost.so")
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def cases(oracle):
    """[(class name, 32-byte encoding)] of every case of tests/compressed_cases.py"""
    classes = cc.g1_classes(oracle)
    assert {"point", "identity", "x>=p", "no point"} <= set(classes)
    big = {int.from_bytes(cc.flagged(c, 0), "big") for c in classes["x>=p"]}
    assert {cc.P, cc.P + 1, (1 << 255) - 1} <= big and {c[0] >> 7 for c in classes["point"]} == {0, 1}
    return [(name, c) for name in sorted(classes) for c in classes[name]]


def inflate_point(hs, c):
    out = ctypes.create_string_buffer(64); inf = ctypes.c_int(0); counts = (ctypes.c_double * 6)()
    ok = hs.hs_kw_inflate_point(c, out, ctypes.byref(inf), counts)
    return ok, out.raw, inf.value, [int(v) for v in counts]


def inflate(hs, c):
    out = ctypes.create_string_buffer(64)
    return hs.hs_kw_inflate(c, out), out.raw


def test_inflate_point_agrees_with_g1_inflate(hs, oracle, cases):
    seen = set()
    for name, c in cases:
        ok, enc, inf, _ = inflate_point(hs, c)
        ok_b, full = inflate(hs, c)
        assert ok == ok_b == (1 if name in ("point", "identity") else 0), (name, c.hex())
        assert inf == (1 if name == "identity" else 0), (name, c.hex())
        if ok:
            assert enc == full == oracle.g1_decompress(c), (name, c.hex())         # the same point after encoding
        else:
            assert full == cc.MARK1 and enc == (1).to_bytes(32, "big") + (2).to_bytes(32, "big"), (name, c.hex())   # the stand-in of th_point
        seen.add((name, ok))
    assert seen == {("point", 1), ("identity", 1), ("x>=p", 0), ("no point", 0)}


def test_identical_operation_counts(hs, cases):
    """a decodable point, the identity and an undecodable input run the same field operations: selects, no branch on data"""
    by_name = {}
    for name, c in cases:
        by_name.setdefault(name, c)
    counts = {name: inflate_point(hs, c)[3] for name, c in by_name.items()}
    assert len(counts) == 4 and counts["point"][1] >= 251                    # the chain's squarings are in it
    assert all(v == counts["point"] for v in counts.values()), counts
    valid = bytes([1, 1, 1, 1])
    idx = np.arange(4, dtype=np.uint32)
    wire = b"".join(by_name[n] for n in ("point", "identity", "x>=p", "no point"))
    scans = []
    for s in range(4):
        pt = ctypes.create_string_buffer(64); cn = (ctypes.c_double * 6)()
        hs.hs_kw_scan_wire(valid, idx.ctypes.data_as(u32p), wire, None, s, pt, cn)
        scans.append([int(v) for v in cn])
    assert all(v == scans[0] for v in scans), scans


def test_scans_agree_with_the_uncompressed_scans_on_the_inflated_bytes(hs, cases):
    wire = [c for _, c in cases]
    n = len(wire)
    full = [inflate(hs, c)[1] for c in wire]
    decodes = [name == "point" for name, _ in cases]
    n_keys = 70
    idx = np.array([(11 * s + 3) % n_keys for s in range(n)], dtype=np.uint32)
    assert n <= n_keys and len(set(idx.tolist())) == n
    key_valid = bytearray([1] * n_keys)
    good = [s for s in range(n) if decodes[s]]
    bad_keys = {int(idx[good[0]]), int(idx[good[5]]), int(idx[good[11]])}    # three points on a bad key
    for k in bad_keys:
        key_valid[k] = 0
    cvalid = np.zeros(3, dtype=np.uint32)
    for k in range(n_keys):
        if key_valid[k]:
            cvalid[k >> 5] |= np.uint32(1 << (k & 31))
    mask = [s % 3 != 1 for s in range(n)]
    want_plain = [int(decodes[s] and key_valid[idx[s]]) for s in range(n)]
    assert 0 in [want_plain[s] for s in range(n) if decodes[s]] and any(decodes[s] and not mask[s] for s in range(n))
    W, F = b"".join(wire), b"".join(full)
    pi = idx.ctypes.data_as(u32p)
    for m, want in ((None, want_plain), (bitmap(mask), [w & int(mask[s]) for s, w in enumerate(want_plain)])):
        for s in range(n):
            a = ctypes.create_string_buffer(64); b = ctypes.create_string_buffer(64); cn = (ctypes.c_double * 6)()
            ca = hs.hs_kw_scan_wire(bytes(key_valid), pi, W, m, s, a, cn)
            cb = hs.hs_kw_scan(bytes(key_valid), pi, F, m, s, b)
            assert ca == cb == want[s], (s, cases[s][0])
            assert a.raw == b.raw == (full[s] if want[s] else IDENT1), (s, cases[s][0])     # canonical form; the identity for a non-candidate
            ca = hs.hs_kw_cscan_wire(cvalid.ctypes.data_as(u32p), pi, W, m, s, a, cn)
            cb = hs.hs_kw_cscan(cvalid.ctypes.data_as(u32p), pi, F, m, s, b)
            assert ca == cb == want[s], (s, cases[s][0])
            assert a.raw == b.raw == (full[s] if want[s] else IDENT1), (s, cases[s][0])


def test_output_is_the_oracles_compression_of_the_affine_sum(hs, oracle, cases):
    pts = [c for name, c in cases if name == "point"]
    junk = [c for name, c in cases if name != "point"]
    for group in ([], pts[:1], pts[:2], pts[2:9], pts[:3] + junk + pts[5:7], [pts[0], cc.flagged(pts[0], 1 - (pts[0][0] >> 7))]):
        kept = [oracle.g1_decompress(c) for c in group if c in pts]
        want = oracle.aggregate_sigs(b"".join(kept), len(kept)) if kept else IDENT1
        full = ctypes.create_string_buffer(64); out = ctypes.create_string_buffer(32)
        hs.hs_kw_sum_out(b"".join(group), len(group), full, out)
        assert full.raw == want, len(group)
        assert out.raw == oracle.g1_compress(want), len(group)
    # P + (-P): the identity, whose compressed form is x = 0 with the parity of y = 1 as the flag
    assert out.raw == bytes([0x80]) + bytes(31) and full.raw == IDENT1
