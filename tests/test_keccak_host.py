"""CPU-only: keccak.h and lane_hash_x.h compiled for the host with -DBN_CHECK (tests/hostsim/keccak_host.cpp) against the model
of tests/expander_support.py, byte for byte: the digests and XOFs over every length 0 .. 400, expand_message for the Keccak-based
expanders at the messages where the pad is one byte or spills into a block of its own, the Z_pad constant, and the lane functions
of k_hash_keccak.hip -- which runs the interval checks over the new path into fp_from_okm.  The same main file, built as a program
of its own with the address and undefined-behaviour sanitizers, is run once as a child process.  A test tool; the product has no CPU path."""
import ctypes
import random
import subprocess

import pytest

from oracle.pyref import bn254 as ref
from tests import expander_support as X
from tests import hostsim_build

DATA = random.Random(1600).randbytes(400)
DSTS = (b"D", b"BLS_SIG_BN254G1_XMD:KECCAK-256_SVDW_RO_NUL_", b"d" * 255, b"e" * 256, b"f" * 300)
assert [len(d) for d in DSTS] == [1, 43, 255, 256, 300]


@pytest.fixture(scope="module")
def hs():
    return ctypes.CDLL(hostsim_build.build("keccak_host.cpp", "libkeccak.so"))


def digest(hs, m, rate, domain, n):
    out = ctypes.create_string_buffer(n)
    hs.hs_kc_hash(m, ctypes.c_size_t(len(m)), rate, domain, out, ctypes.c_size_t(n))
    return out.raw


def staged(hs, xid, dst):
    """the tag as stage_dst leaves it on the device: itself, or the 32 bytes of the oversize rule computed by the header"""
    if len(dst) <= 255:
        return dst
    out = ctypes.create_string_buffer(32)
    hs.hs_kc_oversize_dst(xid, dst, ctypes.c_size_t(len(dst)), out)
    return out.raw


def expand(hs, xid, m, dst, n):
    d = staged(hs, xid, dst)
    out = ctypes.create_string_buffer(n)
    hs.hs_kc_expand(xid, m, ctypes.c_size_t(len(m)), d, len(d), out, n)
    return out.raw


def test_digests_and_xofs_equal_the_model_over_every_length(hs):
    for n in range(401):
        m = DATA[:n]
        assert digest(hs, m, 136, 0x01, 32) == X.keccak256(m), n
        assert digest(hs, m, 136, 0x06, 32) == X.sha3_256(m), n
        for out in (32, 48, 96, 192, 200):
            assert digest(hs, m, 168, 0x1F, out) == X.shake128(m, out), (n, out)
            assert digest(hs, m, 136, 0x1F, out) == X.shake256(m, out), (n, out)


def test_zpad_constant_is_the_permutation_of_zero(hs):
    from tests import library_support  # noqa: F401 (puts scripts/ on the path)
    import keccak_zero_block_state as Z
    got = (ctypes.c_uint64 * 25)()
    hs.hs_kc_zpad_state(got)
    assert list(got) == X.keccak_f([0] * 25) == Z.zero_state()
    st = (ctypes.c_uint64 * 25)()
    hs.hs_kc_f(st)
    assert list(st) == list(got)


@pytest.mark.parametrize("xid", X.IDS[1:])
def test_oversize_rule_equals_the_model(hs, xid):
    for dst in DSTS[3:]:
        assert staged(hs, xid, dst) == X.effective_dst(xid, dst)
    assert staged(hs, X.XMD_SHA256, DSTS[4]) == X.effective_dst(X.XMD_SHA256, DSTS[4])


@pytest.mark.parametrize("xid", X.IDS[1:])
def test_expand_message_equals_the_model_at_the_pad_boundaries(hs, xid):
    for dst in DSTS:
        for m in X.boundary_messages(xid, dst):
            for n in (48, 96, 192):
                assert expand(hs, xid, m, dst, n) == X.expand_message(xid, m, dst, n), (len(dst), len(m), n)


def test_default_id_of_the_dispatcher_is_the_sha256_expander(hs):
    for dst in DSTS:
        assert expand(hs, X.XMD_SHA256, DATA[:77], dst, 96) == ref.expand_message_xmd(DATA[:77], dst, 96)


@pytest.mark.parametrize("xid", X.IDS)
def test_lane_functions_equal_the_model(hs, xid):
    dst = DSTS[1]
    msgs = [DATA[:k] for k in (0, 1, 32, 131, 137, 200)] + [b"abc", DATA]
    assert len(msgs) == 8
    for i, m in enumerate(msgs):
        out = ctypes.create_string_buffer(64)
        for mode, want in ((1, X.hash_to_g1), (3, X.hash_to_g1), (2, X.encode_to_g1)):
            hs.hs_kc_hash_to_g1(xid, m, ctypes.c_size_t(len(m)), dst, len(dst), mode, out)
            assert out.raw == ref.g1_to_bytes(want(xid, m, dst)), (i, mode)
        sc = ctypes.create_string_buffer(32)
        hs.hs_kc_hash_to_scalar(xid, m, ctypes.c_size_t(len(m)), dst, len(dst), sc)
        assert int.from_bytes(sc.raw, "big") == X.hash_to_scalar(xid, m, dst)
    q = ctypes.create_string_buffer(128)                      # G2: the cofactor clearing of the model is the slow part -- two messages
    for m in msgs[3:5]:
        for ro, want in ((1, X.hash_to_g2), (0, X.encode_to_g2)):
            hs.hs_kc_hash_to_g2(xid, m, ctypes.c_size_t(len(m)), dst, len(dst), ro, q)
            assert q.raw == ref.g2_to_bytes(want(xid, m, dst)), ro


def test_sanitized_program_runs_clean(tmp_path_factory):
    """the host code alone, as an ordinary program with its own main: nothing is loaded into this process"""
    exe = tmp_path_factory.mktemp("keccak_host") / "keccak_host"
    prog = hostsim_build.build("keccak_host.cpp", exe, shared=False, extra=hostsim_build.SANITIZED)
    out = subprocess.run([prog], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-1000:], out.stderr[-3000:])
    assert "keccak_host ok" in out.stdout
