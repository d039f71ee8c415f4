"""GPU tests (MI355X) of the operations trimmed from the verify hot path: the lane-per-tuple kernels (k_miller_prepared, k_fe_expx*
with the 12-product chain, k_fe_h3 in its verdict form) forced at small sizes by switching the wave-per-tuple and
three-lanes-per-tuple forms off (BLSBN254_WIDE_FE=0, BLSBN254_TRI_MAX=0), hash_to_g1 with its constant first SHA-256 state and
fixed square-root chain, and the Gt-returning path, which keeps the full last step.  Every expected value is the CPU oracle's."""
import pytest

from tests import synth
from tests.gpu_support import M

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 257)
POOL = 3


@pytest.fixture(scope="module")
def lane_eng(M):
    """an engine whose launches of every size run one lane per tuple"""
    mp = pytest.MonkeyPatch()
    mp.setenv("BLSBN254_WIDE_FE", "0")
    mp.setenv("BLSBN254_TRI_MAX", "0")
    e = M.Engine(0)           # raises when the HIP extension or the GPU is missing: no fallback
    mp.undo()
    yield e
    e.close()


@pytest.fixture(scope="module")
def tuples(oracle, M):
    """257 tuples over a 3-key pool, made once: (keys, key index per tuple, msgs, sigs).  Every fifth tuple is corrupted in a
    rotating way (message bit, another valid signature, another key of the pool); tuple 2 is signed by a fourth key that no other
    tuple uses, so that a launch reads a second table.  20 distinct signed tuples are tiled (signing is CPU work)."""
    dst = M.DEFAULT_DST
    sks = [synth.sk_of(500 + k) for k in range(POOL + 1)]
    keys = [oracle.sk_to_pk(s) for s in sks]
    uniq = [(i % POOL, synth.msg_of(7000 + i)) for i in range(20)]
    signed = [(k, m, oracle.sign(sks[k], m, dst)) for k, m in uniq]
    odd_msg = synth.msg_of(7999)
    odd = (POOL, odd_msg, oracle.sign(sks[POOL], odd_msg, dst))
    g1 = oracle.g1_generator()
    idx, msgs, sigs = [], [], []
    for i in range(max(SIZES)):
        k, m, s = odd if i == 2 else signed[i % 20]
        if i % 5 == 4:
            kind = (i // 5) % 3
            if kind == 0:
                m = bytes([m[0] ^ 1]) + m[1:]
            elif kind == 1:
                s = oracle.g1_add(s, g1)
            else:
                k = (k + 1) % POOL
        idx.append(k); msgs.append(m); sigs.append(s)
    return keys, idx, msgs, sigs


@pytest.mark.parametrize("n", SIZES)
def test_verify_bitmaps_equal_the_oracle(lane_eng, oracle, M, tuples, n):
    """verify_batch_prepared runs k_miller_prepared -> k_fe_easy* -> k_fe_expx* -> k_fe_h3 (one byte per tuple); verify_batch at
    these sizes runs the exact Miller loop in front of the same final exponentiation and k_fe_h3 in its bitmap mode."""
    dst = M.DEFAULT_DST
    keys, idx, msgs, sigs = tuples
    idx, msgs, sigs = idx[:n], msgs[:n], b"".join(sigs[:n])
    pks = b"".join(keys[k] for k in idx)
    want = oracle.verify_batch(pks, msgs, sigs, dst, nthreads=4)
    if n >= 5:
        bits = [(want[i >> 3] >> (i & 7)) & 1 for i in range(n)]
        assert all(bits[i] == (0 if i % 5 == 4 else 1) for i in range(n))
    prep = lane_eng.g2_prepare_batch(b"".join(keys), len(keys))
    try:
        assert lane_eng.verify_batch_prepared(prep, idx, msgs, sigs, dst) == want
    finally:
        prep.close()
    assert lane_eng.verify_batch(pks, msgs, sigs, dst) == want


def test_hash_to_g1_equals_the_oracle(lane_eng, oracle, M):
    """300 messages of lengths 0, 1, 32, 55, 56, 64 and 200 bytes (both sides of the block boundaries of b_0), under the
    default DST and under one of 255 bytes."""
    lengths = (0, 1, 32, 55, 56, 64, 200)
    msgs = [bytes((i * 31 + 7 * k + 1) & 255 for k in range(lengths[i % len(lengths)])) for i in range(300)]
    for dst in (M.DEFAULT_DST, bytes(range(1, 256))):
        assert lane_eng.hash_to_g1_batch(msgs, dst) == oracle.hash_to_g1_batch(msgs, dst)


def test_pairing_batch_keeps_the_full_last_step(lane_eng, oracle):
    """the Gt-returning path: all eight steps of k_fe_h3, bytes equal to the oracle's"""
    g1 = oracle.g1_mul(oracle.g1_generator(), 11) + oracle.g1_mul(oracle.g1_generator(), 12345)
    g2 = oracle.g2_mul(oracle.g2_generator(), 7) + oracle.g2_generator()
    assert lane_eng.pairing_batch(g1, g2, 2) == oracle.pairing_batch(g1, g2, 2)
