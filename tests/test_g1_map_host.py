"""CPU-only: lane_hash_tai.h compiled for the host with -DBN_CHECK (tests/hostsim/g1_map_host.cpp; the common hostsim flags)
against the model of tests/g1_map_support.py, byte for byte: the digests whose reduction matters, messages of other lengths, runs
of 0, 1 and at least 12 skipped candidates, all five plain hashes, and a second build with -DTAI_CAP=4 in which a run of 12
reaches the cap and yields (0, 0).  The same main file, built as a program of its own with the address and undefined-behaviour
sanitizers, is run once as a child process.  A test tool; the product has no CPU path."""
import ctypes
import random
import subprocess

import pytest

from tests import expander_support as X
from tests import g1_map_support as G
from tests import hostsim_build


def bind(path):
    hs = ctypes.CDLL(path)
    hs.hs_tai_hash_to_g1.restype = ctypes.c_int
    return hs


@pytest.fixture(scope="module")
def hs():
    return bind(hostsim_build.build("g1_map_host.cpp", "libg1map.so"))


@pytest.fixture(scope="module")
def hs_cap4():
    return bind(hostsim_build.build("g1_map_host.cpp", "libg1map_cap4.so", extra=["-DTAI_CAP=4"]))


def hashed(hs, map_id, xid, m):
    out = ctypes.create_string_buffer(64)
    k = hs.hs_tai_hash_to_g1(map_id, xid, m, ctypes.c_size_t(len(m)), out)
    return out.raw, k


def test_the_library_cap(hs, hs_cap4):
    assert hs.hs_tai_cap() == G.CAP and hs_cap4.hs_tai_cap() == 4


def test_edge_digests_and_other_lengths(hs):
    for m in G.EDGE_DIGESTS + G.ODD_LENGTHS + [(G.P - 2).to_bytes(32, "big")]:
        x0 = ctypes.create_string_buffer(32)
        hs.hs_tai_x0(G.TAI_DIGEST, 0, m, ctypes.c_size_t(len(m)), x0)
        assert int.from_bytes(x0.raw, "big") == G.x0_of(G.TAI_DIGEST, 0, m), m.hex()
        got, k = hashed(hs, G.TAI_DIGEST, 0, m)
        assert got == G.hash_bytes(G.TAI_DIGEST, 0, m) and k == G.run_of(G.x0_of(G.TAI_DIGEST, 0, m)), m.hex()


@pytest.mark.parametrize("run,at_least", [(0, False), (1, False), (2, False), (5, False), (12, True)])
def test_prescribed_runs(hs, run, at_least):
    for d in G.digests_with_run(run, 3, at_least=at_least):
        got, k = hashed(hs, G.TAI_DIGEST, 0, d)
        want, kw = G.contract_loop(int.from_bytes(d, "big"))
        assert (k >= run if at_least else k == run) and k == kw
        assert got == G.point_bytes(want) and G.holds(int.from_bytes(d, "big"), want, k)


@pytest.mark.parametrize("xid", X.IDS)
def test_plain_hashes(hs, xid):
    rnd = random.Random(90 + xid)
    for ln in (0, 1, 32, 55, 56, 64, 135, 136, 137, 167, 168, 200):
        m = rnd.randbytes(ln)
        d = ctypes.create_string_buffer(32)
        hs.hs_tai_digest(xid, m, ctypes.c_size_t(ln), d)
        assert d.raw == G.PLAIN[xid](m), ln
        assert hashed(hs, G.TAI_HASH, xid, m)[0] == G.hash_bytes(G.TAI_HASH, xid, m), ln
        out = ctypes.create_string_buffer(64)
        hs.hs_tai_lane(G.TAI_HASH, xid, m, ctypes.c_size_t(ln), out)
        assert out.raw == G.hash_bytes(G.TAI_HASH, xid, m), ln


def test_the_cap_is_reached_at_four(hs, hs_cap4):
    long_run = G.digests_with_run(12, 1, at_least=True)[0]
    assert hashed(hs_cap4, G.TAI_DIGEST, 0, long_run) == (bytes(64), 4) == (G.hash_bytes(G.TAI_DIGEST, 0, long_run, cap=4), 4)
    assert hashed(hs, G.TAI_DIGEST, 0, long_run)[0] == G.hash_bytes(G.TAI_DIGEST, 0, long_run) != bytes(64)
    for run in (0, 3):                                   # below the cap the small build is the library
        d = G.digests_with_run(run, 1)[0]
        assert hashed(hs_cap4, G.TAI_DIGEST, 0, d) == (G.hash_bytes(G.TAI_DIGEST, 0, d), run)
    d4 = G.digests_with_run(4, 1)[0]                      # the first run the small cap refuses
    assert hashed(hs_cap4, G.TAI_DIGEST, 0, d4) == (bytes(64), 4)


def test_sanitized_program_runs_clean(tmp_path_factory):
    """the lane functions alone, as an ordinary program with its own main: nothing is loaded into this process.  The common
    recipe plus the sanitizers; -fno-sanitize=shift because the field code shifts signed limbs left by design (fp29.h fp_lc)"""
    exe = tmp_path_factory.mktemp("g1_map_host") / "g1_map_host"
    prog = hostsim_build.build("g1_map_host.cpp", exe, shared=False, extra=hostsim_build.SANITIZED + ["-fno-sanitize=shift"])
    out = subprocess.run([prog], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stdout[-1000:], out.stderr[-3000:])
    assert "g1_map_host ok" in out.stdout
