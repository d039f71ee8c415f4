"""GPU tests (MI355X) of the pairing-product equations over ragged groups of pairs (blsbn254_multi_miller_loop_batch /
blsbn254_pairing_check_batch): Miller products against the oracle's multi_miller_loop and the library's own, check bits against
the oracle's final exponentiation combined with its point checks, closed-form equations (P_j = [a_j] G1, Q_j = [b_j] G2 holds
iff sum_j a_j b_j = 0 mod r), invalid members, the BLS verify equation, every launch form and chunking, a large batch and the
argument errors."""
import ctypes
import random

import numpy as np
import pytest

from tests import synth
from tests.gpu_support import eng, M
from tests.helpers import b32, bits_of, IDENT1, IDENT2, offsets_u64

pytestmark = pytest.mark.gpu
R = synth.R
ONE = (1).to_bytes(32, "big") + bytes(352)                       # Fp12::ONE
E_ARG = -1


def closed_form_scalars(rnd, sizes, holds, zero=()):
    """a, b per pair and whether each equation holds: equation g's sum a_j b_j is 0 mod r when holds[g] (else 1).  Pairs listed in
    `zero` (global indices) get a = 0 (an identity P); the last pair with a non-zero a absorbs the sum, and an equation without
    one holds whatever holds[g] says."""
    a, b, actual = [], [], []
    zero = set(zero)
    pos = 0
    for g, k in enumerate(sizes):
        ag = [0 if pos + j in zero else rnd.randrange(1, R) for j in range(k)]
        bg = [rnd.randrange(1, R) for _ in range(k)]
        nz = [j for j in range(k) if ag[j]]
        if nz:
            last = nz[-1]
            rest = sum(ag[j] * bg[j] for j in range(k) if j != last) % R
            want = 0 if holds[g] else 1
            bg[last] = (want - rest) * pow(ag[last], -1, R) % R
        a += ag; b += bg; pos += k
        actual.append(bool(holds[g]) if nz else True)
    return a, b, actual


def points_gpu(eng, oracle, a, b):
    n = len(a)
    if n == 0:
        return b"", b""
    G1, G2 = oracle.g1_generator(), oracle.g2_generator()
    P = eng.g1_mul_batch(G1 * n, b"".join(map(b32, a)), n)
    Q = eng.g2_mul_batch(G2 * n, b"".join(map(b32, b)), n)
    return P, Q


def truth(oracle, g1, g2, off):
    """(Miller products or None where a point does not decode, check bits) composed from the oracle: multi_miller_loop,
    final_exponentiation, g1_check_batch / g2_check_batch, with the identity handled explicitly."""
    mls, bits = [], []
    for g in range(len(off) - 1):
        lo, hi = int(off[g]), int(off[g + 1])
        k = hi - lo
        P, Q = g1[64 * lo:64 * hi], g2[128 * lo:128 * hi]
        try:
            ml = oracle.multi_miller_loop(P, Q, k) if k else ONE
        except Exception:
            ml = None
        ok = ml is not None
        if k and ok:
            c1, c2 = oracle.g1_check_batch(P, k), oracle.g2_check_batch(Q, k)
            for j in range(k):
                id1 = P[64 * j:64 * j + 32] == bytes(32)
                id2 = Q[128 * j:128 * j + 64] == bytes(64)
                ok &= (id1 or bool(c1[j >> 3] >> (j & 7) & 1)) and (id2 or bool(c2[j >> 3] >> (j & 7) & 1))
        mls.append(ml)
        bits.append(ok and oracle.final_exponentiation(ml, 1) == ONE)
    return mls, bits


# ---------------------------------------------------------------- 1. small ragged batches against the oracle
def test_small_ragged_vs_oracle(eng, oracle):
    rnd = random.Random(1)
    sizes = [0, 1, 2, 3, 4, 7, 33, 2, 4, 3]
    holds = [True, False, True, True, True, False, True, False, True, True]
    zero = [3, 6 + 1, 10 + 2, 50]                                # a few identity P members
    a, b, _ = closed_form_scalars(rnd, sizes, holds, zero)
    P, Q = points_gpu(eng, oracle, a, b)
    Q = bytearray(Q)
    Q[128 * 4:128 * 5] = IDENT2                                  # an identity Q in the 3-pair group (its equation no longer holds)
    Q = bytes(Q)
    off = offsets_u64(sizes)
    mls, bits = truth(oracle, P, Q, off)
    got = eng.multi_miller_loop_batch(P, Q, off)
    assert len(got) == 384 * len(sizes)
    for g in range(len(sizes)):
        lo, hi = int(off[g]), int(off[g + 1])
        assert got[384 * g:384 * g + 384] == mls[g], g
        assert got[384 * g:384 * g + 384] == eng.multi_miller_loop(P[64 * lo:64 * hi], Q[128 * lo:128 * hi], hi - lo), g
    bm = eng.pairing_check_batch(P, Q, off)
    assert bits_of(bm, len(sizes)) == bits
    assert bits[0] and bits[2] and not bits[1] and not bits[3]    # the closed form agrees with the oracle's composition


def test_offsets_need_not_start_at_zero(eng, oracle):
    rnd = random.Random(2)
    sizes = [2, 0, 3]
    a, b, _ = closed_form_scalars(rnd, [1] + sizes, [False, True, True, False])
    P, Q = points_gpu(eng, oracle, a, b)
    off = offsets_u64([1] + sizes)[1:]                                  # the first pair belongs to no equation
    out = np.zeros(1, dtype=np.uint8)
    o = np.ascontiguousarray(off)
    g1 = np.frombuffer(P, dtype=np.uint8); g2 = np.frombuffer(Q, dtype=np.uint8)
    u8 = ctypes.POINTER(ctypes.c_uint8)
    rc = eng._lib.blsbn254_pairing_check_batch(eng._ctx, g1.ctypes.data_as(u8), g2.ctypes.data_as(u8), o.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                               ctypes.c_size_t(3), out.ctypes.data_as(u8))
    assert rc == 0 and bits_of(out.tobytes(), 3) == [True, True, False]


# ---------------------------------------------------------------- 2. closed-form equations
def test_closed_form_shapes(eng, oracle):
    rnd = random.Random(3)
    # KZG shape (2 pairs) and Groth16 shape (4 pairs), holding and off by one
    sizes = [2, 2, 4, 4] * 8
    holds = [True, False, True, False] * 8
    a, b, _ = closed_form_scalars(rnd, sizes, holds)
    P, Q = points_gpu(eng, oracle, a, b)
    assert bits_of(eng.pairing_check_batch(P, Q, offsets_u64(sizes)), len(sizes)) == holds


def test_identity_members(eng, oracle):
    rnd = random.Random(4)
    G1, G2 = oracle.g1_generator(), oracle.g2_generator()
    Pa = oracle.g1_mul(G1, rnd.randrange(1, R)); Qb = oracle.g2_mul(G2, rnd.randrange(1, R))
    eqs = [
        ([(IDENT1, Qb), (Pa, IDENT2)], True),                        # holds only because every pair has an identity member
        ([(IDENT1, IDENT2), (IDENT1, IDENT2)], True),                # all pairs identity
        ([(IDENT1, IDENT2)], True),
        ([(Pa, Qb), (IDENT1, Qb)], False),                           # one real pair left: e(Pa, Qb) != 1
        ([(Pa, Qb), (oracle.g1_mul(Pa, R - 1), Qb), (Pa, IDENT2)], True),
    ]
    P = b"".join(p for eq, _ in eqs for p, _ in eq)
    Q = b"".join(q for eq, _ in eqs for _, q in eq)
    off = offsets_u64([len(eq) for eq, _ in eqs])
    want = [h for _, h in eqs]
    assert bits_of(eng.pairing_check_batch(P, Q, off), len(eqs)) == want
    assert truth(oracle, P, Q, off)[1] == want
    ml = eng.multi_miller_loop_batch(P, Q, off)
    assert ml[384:768] == ONE and ml[768:1152] == ONE


# ---------------------------------------------------------------- 3. invalid members clear exactly their equation's bit
def test_invalid_members(eng, oracle, M):
    rnd = random.Random(5)
    n_eq = 12                                                        # equation g: pairs 2g, 2g + 1, all holding before the damage
    a, b, _ = closed_form_scalars(rnd, [2] * n_eq, [True] * n_eq)
    P, Q = points_gpu(eng, oracle, a, b)
    P, Q = bytearray(P), bytearray(Q)
    P[64 * 2:64 * 2 + 32] = b"\xff" * 32                            # eq 1: P does not decode (x >= p)
    P[64 * 5 + 63] ^= 1                                              # eq 2: P off the curve
    Q[128 * 6 + 127] ^= 1                                            # eq 3: Q off the curve
    # eq 5: (O, T) and (P, O) with T on the curve outside the r-torsion: both pairs are skipped, the product is 1
    P[64 * 10:64 * 11] = IDENT1
    Q[128 * 10:128 * 11] = synth.NON_SUBGROUP_PK
    Q[128 * 11:128 * 12] = IDENT2
    Q[128 * 14:128 * 14 + 32] = b"\xff" * 32                        # eq 7: Q does not decode (x.c1 >= p)
    P, Q = bytes(P), bytes(Q)
    off = offsets_u64([2] * n_eq)
    want = [g not in (1, 2, 3, 5, 7) for g in range(n_eq)]
    mls, tb = truth(oracle, P, Q, off)
    assert tb == want
    assert mls[5] == ONE                                             # it would cancel to 1 but for the torsion test
    assert bits_of(eng.pairing_check_batch(P, Q, off), n_eq) == want
    # the Miller products: a point that does not decode is an error, as in multi_miller_loop; the other bad points are not
    with pytest.raises(M.InvalidG1Bytes):
        eng.multi_miller_loop_batch(P, Q, off)
    assert "pair 2" in eng._lib.blsbn254_last_error(eng._ctx).decode()
    P = P[:64 * 2] + IDENT1 + P[64 * 3:]
    with pytest.raises(M.InvalidG2Bytes):
        eng.multi_miller_loop_batch(P, Q, off)
    assert "pair 14" in eng._lib.blsbn254_last_error(eng._ctx).decode()
    Q = Q[:128 * 14] + IDENT2 + Q[128 * 15:]
    ml = eng.multi_miller_loop_batch(P, Q, off)
    for g in range(n_eq):
        assert ml[384 * g:384 * g + 384] == eng.multi_miller_loop(P[128 * g:128 * g + 128], Q[256 * g:256 * g + 256], 2), g
        assert ml[384 * g:384 * g + 384] == oracle.multi_miller_loop(P[128 * g:128 * g + 128], Q[256 * g:256 * g + 256], 2), g


# ---------------------------------------------------------------- 4. BLS equivalence
def test_bls_verify_equivalence(eng, oracle, M):
    dst = M.DEFAULT_DST
    n = 640
    pks, msgs, sigs, exp = synth.make_batch(oracle, n, dst, invalid_every=64, uniq=64)
    H = eng.hash_to_g1_batch(msgs, dst)
    neg_g2 = oracle.g2_mul(oracle.g2_generator(), R - 1)
    P = b"".join(sigs[64 * i:64 * i + 64] + H[64 * i:64 * i + 64] for i in range(n))
    Q = b"".join(neg_g2 + pks[128 * i:128 * i + 128] for i in range(n))
    got = eng.pairing_check_batch(P, Q, offsets_u64([2] * n))
    assert got == eng.verify_batch(pks, msgs, sigs, dst) == synth.bitmap_of(exp)


# ---------------------------------------------------------------- 5. launch forms and chunking
def _ragged(rnd, n_eq, lo, hi):
    sizes = [rnd.randint(lo, hi) for _ in range(n_eq)]
    holds = [rnd.random() < 0.7 for _ in range(n_eq)]
    return sizes, holds


def _run_forms(M, eng, oracle, monkeypatch, sizes, holds, seed, envs):
    rnd = random.Random(seed)
    a, b, holds = closed_form_scalars(rnd, sizes, holds, zero=[i for i in range(sum(sizes)) if i % 37 == 5])
    P, Q = points_gpu(eng, oracle, a, b)
    off = offsets_u64(sizes)
    bm = eng.pairing_check_batch(P, Q, off)
    ml = eng.multi_miller_loop_batch(P, Q, off)
    assert bits_of(bm, len(sizes)) == holds
    for g in sorted({0, len(sizes) // 2, len(sizes) - 1}):
        lo, hi = int(off[g]), int(off[g + 1])
        assert ml[384 * g:384 * g + 384] == oracle.multi_miller_loop(P[64 * lo:64 * hi], Q[128 * lo:128 * hi], hi - lo), g
    for env in envs:
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            e2 = M.Engine(0)
            try:
                assert e2.pairing_check_batch(P, Q, off) == bm, env
                assert e2.multi_miller_loop_batch(P, Q, off) == ml, env
            finally:
                e2.close()


ENVS = [{"BLSBN254_WIDE_FE": "0"}, {"BLSBN254_TRI_MAX": "0"}, {"BLSBN254_WIDE_FE": "0", "BLSBN254_TRI_MAX": "0"}]


def test_wide_form(M, eng, oracle, monkeypatch):
    sizes, holds = _ragged(random.Random(10), 300, 1, 5)            # <= 1024 pairs: one wave per pair
    assert sum(sizes) <= 1024
    _run_forms(M, eng, oracle, monkeypatch, sizes, holds, 11, ENVS)


def test_tri_form(M, eng, oracle, monkeypatch):
    sizes, holds = _ragged(random.Random(12), 2500, 1, 4)           # 1024 < pairs <= 16384: four lanes per pair
    assert 1024 < sum(sizes) <= 16384
    _run_forms(M, eng, oracle, monkeypatch, sizes, holds, 13, ENVS)


def test_lane_form(M, eng, oracle, monkeypatch):
    sizes, holds = _ragged(random.Random(14), 8000, 1, 4)           # > 16384 pairs: one lane per pair
    assert sum(sizes) > 16384
    _run_forms(M, eng, oracle, monkeypatch, sizes, holds, 15, ENVS[:1])


def test_chunking_straddles_and_exceeds_a_chunk(M, eng, oracle, monkeypatch):
    rnd = random.Random(16)
    sizes, holds = _ragged(rnd, 60, 1, 150)
    sizes[3:3] = [0, 0]; holds[3:3] = [True, True]                   # empty equations in the middle, and at the end
    sizes += [0]; holds += [True]
    _run_forms(M, eng, oracle, monkeypatch, sizes, holds, 17, [{"BLSBN254_CHUNK_LANES": "64"}, {"BLSBN254_CHUNK_LANES": "8"}])


def test_one_huge_equation(M, eng, oracle, monkeypatch):
    _run_forms(M, eng, oracle, monkeypatch, [5000], [True], 18, [{"BLSBN254_CHUNK_LANES": "512"}])
    _run_forms(M, eng, oracle, monkeypatch, [1, 5000, 2], [False, True, True], 19, [{"BLSBN254_CHUNK_LANES": "512"}])


# ---------------------------------------------------------------- 6. large batch
def test_large_two_pair_equations(eng, oracle):
    rnd = random.Random(20)
    n_eq = 1 << 18
    a0 = [rnd.randrange(1, R) for _ in range(n_eq)]; b0 = [rnd.randrange(1, R) for _ in range(n_eq)]
    a1 = [rnd.randrange(1, R) for _ in range(n_eq)]
    b1 = [(-x * y) * pow(z, -1, R) % R for x, y, z in zip(a0, b0, a1)]
    holds = [True] * n_eq
    for g in range(63, n_eq, 64):                                    # 1/64 broken by one scalar
        b0[g] = (b0[g] + 1) % R
        holds[g] = False
    a = [v for pair in zip(a0, a1) for v in pair]; b = [v for pair in zip(b0, b1) for v in pair]
    P, Q = points_gpu(eng, oracle, a, b)
    got = eng.pairing_check_batch(P, Q, offsets_u64([2] * n_eq))
    assert got == synth.bitmap_of(holds)


# ---------------------------------------------------------------- 7. argument errors
def test_argument_errors(eng, oracle):
    lib, ctx = eng._lib, eng._ctx
    u8 = ctypes.POINTER(ctypes.c_uint8); u64 = ctypes.POINTER(ctypes.c_uint64)
    G1, G2 = oracle.g1_generator(), oracle.g2_generator()
    g1 = np.frombuffer(G1 * 4, dtype=np.uint8); g2 = np.frombuffer(G2 * 4, dtype=np.uint8)
    out = np.zeros(384 * 4, dtype=np.uint8)
    p1, p2, po = g1.ctypes.data_as(u8), g2.ctypes.data_as(u8), out.ctypes.data_as(u8)

    def call(fn, off, n, a=p1, b=p2, o=po):
        arr = np.ascontiguousarray(np.asarray(off, dtype=np.uint64))
        return fn(ctx, a, b, arr.ctypes.data_as(u64) if len(off) else None, ctypes.c_size_t(n), o)

    for fn in (lib.blsbn254_pairing_check_batch, lib.blsbn254_multi_miller_loop_batch):
        assert call(fn, [0, 3, 1], 2) == E_ARG                       # decreasing offsets
        assert call(fn, [0, (1 << 23) + 1], 1) == E_ARG              # more than 2^23 pairs
        assert call(fn, [0, 2], 1, a=None) == E_ARG
        assert call(fn, [0, 2], 1, b=None) == E_ARG
        assert call(fn, [0, 2], 1, o=None) == E_ARG
        assert call(fn, [], 1) == E_ARG                              # no offsets
        assert call(fn, [0], 0) == 0 and call(fn, [], 0, a=None, b=None, o=None) == 0
        assert call(fn, [0, 2, 4], 2) == 0
    assert eng.pairing_check_batch(b"", b"", [0]) == b""
    assert eng.multi_miller_loop_batch(b"", b"", [0, 0]) == ONE
    assert eng.pairing_check_batch(b"", b"", [0, 0, 0]) == b"\x03"
