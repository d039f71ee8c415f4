"""CPU-only: tests/expander_support.py is what every expander test compares the device and host code with, so it is pinned
first -- its SHA-3 and SHAKE against hashlib over every length that crosses both rates twice, its Keccak-256 (same permutation and
sponge, another domain byte) against two published digests, and its expand_message against the default expander of
oracle/pyref/bn254.py and against RFC 9380's framing written out directly over hashlib."""
import hashlib
import random

import pytest

from oracle.pyref import bn254 as ref
from tests import expander_support as X

DATA = random.Random(202).randbytes(400)
DSTS = (b"D", b"QUUX-V01-CS02-with-BN254G1_XMD:KECCAK-256_SVDW_RO_", b"d" * 255, b"e" * 256, b"f" * 300)
MSGS = (b"", b"abc", DATA[:131], DATA[:137], DATA)


def test_sha3_and_shake_equal_hashlib_over_every_length():
    for n in range(401):
        m = DATA[:n]
        assert X.sha3_256(m) == hashlib.sha3_256(m).digest(), n
        for out in (32, 48, 96, 192, 200):
            assert X.shake128(m, out) == hashlib.shake_128(m).digest(out), (n, out)
            assert X.shake256(m, out) == hashlib.shake_256(m).digest(out), (n, out)


def test_keccak256_equals_the_published_digests():
    assert X.keccak256(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    assert X.keccak256(b"abc").hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"


def test_zero_state_script_agrees_with_the_model():
    from tests import library_support  # noqa: F401 (puts scripts/ on the path)
    import keccak_zero_block_state as Z
    assert Z.zero_state() == X.keccak_f([0] * 25)
    assert X.sponge(136, 0x06, b"", 32) == hashlib.sha3_256(b"").digest()


@pytest.mark.parametrize("n", (48, 96, 192))
def test_default_expander_equals_pyref(n):
    for dst in DSTS:
        for m in MSGS:
            assert X.expand_message(X.XMD_SHA256, m, dst, n) == ref.expand_message_xmd(m, dst, n)


def xmd_direct(h, s_in_bytes, msg, dst, n):
    """RFC 9380 5.3.1 and 5.3.3 over a 32-byte hash h(bytes) -> bytes, written out on its own"""
    if len(dst) > 255:
        dst = h(b"H2C-OVERSIZE-DST-" + dst)
    dp = dst + len(dst).to_bytes(1, "big")
    b0 = h(bytes(s_in_bytes) + msg + n.to_bytes(2, "big") + b"\0" + dp)
    b = [h(b0 + b"\x01" + dp)]
    for i in range(2, -(-n // 32) + 1):
        b.append(h(bytes(x ^ y for x, y in zip(b0, b[-1])) + bytes([i]) + dp))
    return b"".join(b)[:n]


def xof_direct(h, msg, dst, n):
    """RFC 9380 5.3.2 and 5.3.3 (k = 128: 32 bytes) over a hashlib XOF"""
    if len(dst) > 255:
        dst = h(b"H2C-OVERSIZE-DST-" + dst).digest(32)
    return h(msg + n.to_bytes(2, "big") + dst + bytes([len(dst)])).digest(n)


@pytest.mark.parametrize("n", (48, 96, 192))
def test_sha3_and_shake_expanders_equal_the_framing_over_hashlib(n):
    for dst in DSTS:
        for m in MSGS:
            assert X.expand_message(X.XMD_SHA3_256, m, dst, n) == xmd_direct(lambda b: hashlib.sha3_256(b).digest(), 136, m, dst, n)
            assert X.expand_message(X.XOF_SHAKE128, m, dst, n) == xof_direct(hashlib.shake_128, m, dst, n)
            assert X.expand_message(X.XOF_SHAKE256, m, dst, n) == xof_direct(hashlib.shake_256, m, dst, n)


def test_keccak_expander_differs_from_sha3_only_through_the_domain_byte():
    """id 1 is id 2's code path with 0x01 in place of 0x06: the same framing over the model's own keccak256"""
    for dst in DSTS:
        for m in MSGS:
            want = xmd_direct(X.keccak256, 136, m, dst, 96)
            assert X.expand_message(X.XMD_KECCAK256, m, dst, 96) == want
            assert want != X.expand_message(X.XMD_SHA3_256, m, dst, 96)


def test_boundary_messages_hit_the_pad_cases():
    for xid in X.IDS[1:]:
        rate = 168 if xid == X.XOF_SHAKE128 else 136
        for dst in DSTS:
            dl = len(X.effective_dst(xid, dst))
            got = []
            for m in X.boundary_messages(xid, dst)[:4]:
                absorbed = len(m) + 2 + dl + 1 + (0 if xid in X.XOF_HASH else rate + 1)
                got.append(absorbed % rate)
            assert got == [0, 1, rate - 2, rate - 1]


def test_hash_to_field_and_curve_compose_the_pinned_maps():
    dst = DSTS[1]
    for xid in X.IDS:
        u = X.hash_to_fp(xid, b"m", dst, 2)
        assert ref.g1_on_curve(X.hash_to_g1(xid, b"m", dst)) and X.hash_to_g1(xid, b"m", dst) == ref.g1_add(ref.svdw_g1(u[0]), ref.svdw_g1(u[1]))
        assert 0 <= X.hash_to_scalar(xid, b"m", dst) < ref.R
    assert X.hash_to_g1(X.XMD_SHA256, b"m", dst) == ref.hash_to_g1(b"m", dst)
    assert X.hash_to_scalar(X.XMD_SHA256, b"m", dst) == ref.hash_to_scalar(b"m", dst)
    assert X.sign(X.XMD_SHA256, 12345, b"m", dst) == ref.sign(12345, b"m", dst)
