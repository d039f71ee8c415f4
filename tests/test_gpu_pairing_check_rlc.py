"""GPU tests (MI355X) of the pairing-product checks over ragged groups by random linear combination across equations
(blsbn254_pairing_check_batch_rlc): every bitmap is compared with blsbn254_pairing_check_batch on the same arguments and with the
truth known by construction (P = [a] G1gen, Q = [b] G2gen with b from a small pool: an equation holds iff sum a_j b_j = 0 mod r),
and every case asserts what the counters of the call say, so that equality is never reached merely through the exact sub-call."""
import ctypes
import random

import numpy as np
import pytest

from tests import synth
from tests.aggregate_rlc_support import Data
from tests.gpu_support import MILLER_KERNELS, eng, engines, fresh_engine, launches, M  # noqa: F401 (fixtures)
from tests.helpers import IDENT1, IDENT2, b32, bits_of, offsets_u64
from tests.pairing_check_rlc_support import PCR_STATS, SEED, closed_form, points

pytestmark = pytest.mark.gpu
R, P_MOD = synth.R, synth.P
ONE = (1).to_bytes(32, "big") + bytes(352)                       # Fp12::ONE
E_ARG = -1
SEED_B = bytes(range(7, 39))
VARIABLE_Q = ("miller_wide_1", "miller_tri_1", "miller_1")       # the Miller kernels of the exact call
POOL = (31337, 4242, R - 5)                                      # the scalars of the three distinct Q


def run(e, g1, g2, off, seed=SEED):
    """(bits of the RLC call, what its counters moved by); the bitmap equals the exact call's on the same arguments"""
    n_eq = len(off) - 1
    s0 = e.pairing_check_rlc_stats()
    got = e.pairing_check_batch_rlc(g1, g2, off, seed)
    s1 = e.pairing_check_rlc_stats()
    assert got == e.pairing_check_batch(g1, g2, off)
    return bits_of(got, n_eq), {k: s1[k] - s0[k] for k in PCR_STATS}


def stats(calls=1, round1=0, round2=0, exact=0, ineligible=0, equations=1, exact_calls=0, failed=0):
    return dict(zip(PCR_STATS, (calls, round1, round2, exact, ineligible, equations, exact_calls, failed)))


def batch(e, oracle, seed, sizes, holds, zero=(), pool=POOL):
    a, kk, actual = closed_form(random.Random(seed), sizes, holds, pool, zero)
    g1, g2 = points(e, oracle, a, kk, pool)
    return g1, g2, actual


# ---------------------------------------------------------------- 1. honest ragged batch
def test_honest_ragged_batch(engines, oracle):
    sizes = [2, 2, 0, 3, 1, 4, 9, 2] * 3
    zero = [i * 23 + 7 for i in range(3)]                          # the one-pair equations: an identity P
    eng = engines["default"]
    g1, g2, actual = batch(eng, oracle, 1, sizes, [True] * len(sizes), zero)
    off = offsets_u64(sizes)
    assert actual == [True] * len(sizes) and all(g1[64 * z:64 * z + 64] == IDENT1 for z in zero)
    for name in ("default", "tri", "lane"):
        e = engines[name]
        bits, delta = run(e, g1, g2, off)
        assert bits == actual, name
        assert delta == stats(round1=len(sizes)), name                # one combined equation decided everything
        got, rec = launches(e, lambda: e.pairing_check_batch_rlc(g1, g2, off, SEED), MILLER_KERNELS)
        assert bits_of(got, len(sizes)) == actual
        assert not [k for k in VARIABLE_Q if k in rec] and sum(rec.values()) == 1, (name, rec)      # 3 table-only slots in one launch


# ---------------------------------------------------------------- 2. damage classes
def test_damage_classes_clear_their_equations_only(eng, oracle):
    n_eq = 12
    holds = [g != 1 for g in range(n_eq)]                               # equation 1: false
    g1, g2, actual = batch(eng, oracle, 2, [2] * n_eq, holds)
    g1, g2 = bytearray(g1), bytearray(g2)
    g1[64 * 4 + 63] ^= 1                                                # equation 2: P off the curve
    g1[64 * 7:64 * 7 + 32] = b32(P_MOD + 1)                            # equation 3: a P coordinate >= p
    g2[128 * 10 + 127] ^= 1                                             # equation 5: Q off the curve
    g2[128 * 15:128 * 16] = synth.NON_SUBGROUP_PK                      # equation 7: Q outside the r-torsion
    g2[128 * 18 + 32:128 * 18 + 64] = b"\xff" * 32                     # equation 9: a Q coordinate >= p
    g1, g2 = bytes(g1), bytes(g2)
    want = [g not in (1, 2, 3, 5, 7, 9) for g in range(n_eq)]
    bits, delta = run(eng, g1, g2, offsets_u64([2] * n_eq))             # never an error
    assert bits == want
    assert delta["ineligible_equations"] == 5 and delta["round1_equations"] == 0
    # 6 distinct Q among 24 pairs: two segments of 6 equations; the first holds equation 1 and fails, its eligible equations 0, 1, 4
    # go to the exact call; the second passes with its eligible equations 6, 8, 10, 11
    assert delta == stats(round2=4, exact=3, ineligible=5, equations=3, failed=1)


# ---------------------------------------------------------------- 3. skipped pairs, trivial equations
def test_skipped_pairs_and_trivial_equations(eng, oracle):
    rnd = random.Random(3)
    G1, G2 = oracle.g1_generator(), oracle.g2_generator()
    k = rnd.randrange(1, R)
    Pa, Qb = oracle.g1_mul(G1, k), oracle.g2_mul(G2, POOL[0])
    nPa = oracle.g1_mul(G1, R - k)
    ident2_y = bytes(64) + b32(5) + b32(9)                              # the identity by its encoding, whatever y is
    eqs = [
        ([(IDENT1, Qb), (Pa, IDENT2)], True),                           # identity pairs only
        ([], True),
        ([(Pa, Qb), (nPa, Qb), (Pa, IDENT2), (IDENT1, Qb)], True),      # still holds with identity P and identity Q inside
        ([(Pa, Qb), (IDENT1, Qb)], False),                              # still fails: e(Pa, Qb) is left
        ([(Pa, Qb), (nPa, Qb), (bytes(32) + b32(7), Qb), (nPa, ident2_y)], True),
        ([(IDENT1, IDENT2)], True),
        ([(Pa, Qb), (Pa, Qb), (nPa, IDENT2)], False),
        ([], True),
    ]
    g1 = b"".join(p for eq, _ in eqs for p, _ in eq)
    g2 = b"".join(q for eq, _ in eqs for _, q in eq)
    want = [h for _, h in eqs]
    bits, delta = run(eng, g1, g2, offsets_u64([len(eq) for eq, _ in eqs]))
    assert bits == want
    assert delta["ineligible_equations"] == 0 and delta["exact_calls"] == 0 and delta["round1_equations"] == 0
    # without the two false equations everything is decided by round 1
    good = [eq for eq, h in eqs if h]
    bits, delta = run(eng, b"".join(p for eq in good for p, _ in eq), b"".join(q for eq in good for _, q in eq), offsets_u64([len(eq) for eq in good]))
    assert bits == [True] * len(good) and delta == stats(round1=len(good))


# ---------------------------------------------------------------- 4. errors that cancel without weights
def test_cancelling_errors(eng, oracle):
    G1, G2 = oracle.g1_generator(), oracle.g2_generator()
    q, q2, a, t = POOL[0], POOL[1], 1234567, 777
    Q, Q2 = oracle.g2_mul(G2, q), oracle.g2_mul(G2, q2)
    A, nA = oracle.g1_mul(G1, a), oracle.g1_mul(G1, (-a * q2 * pow(q, -1, R)) % R)      # e(A, Q2) e(nA, Q) = 1
    T, nT = oracle.g1_mul(G1, t), oracle.g1_mul(G1, R - t)
    eqs = [[(A, Q2), (nA, Q), (T, Q)], [(nA, Q), (A, Q2), (nT, Q)], [(A, Q2), (nA, Q)]]
    g1 = b"".join(p for eq in eqs for p, _ in eq)
    g2 = b"".join(q_ for eq in eqs for _, q_ in eq)
    off = offsets_u64([3, 3, 2])
    for seed in (SEED, SEED_B):
        bits, delta = run(eng, g1, g2, off, seed)
        assert bits == [False, False, True]
        assert delta["round1_equations"] == 0 and delta["ineligible_equations"] == 0
    # the two false equations multiply to one without weights
    ml = eng.multi_miller_loop_batch(g1[:64 * 6], g2[:128 * 6], [0, 6])
    assert eng.final_exponentiation(ml) == ONE
    for lo, hi in ((0, 3), (3, 6)):
        assert eng.final_exponentiation(eng.multi_miller_loop_batch(g1[64 * lo:64 * hi], g2[128 * lo:128 * hi], [0, 3])) != ONE


# ---------------------------------------------------------------- 5. all Q distinct: the call is the exact call
def test_all_distinct_q_is_the_exact_call(eng, oracle):
    pool = tuple(range(1000, 1008))
    sizes, holds = [2] * 4, [True, False, True, True]
    rnd = random.Random(5)
    a = [rnd.randrange(1, R) for _ in range(8)]
    for g in range(4):                                                  # a_0 b_0 + a_1 b_1 = 0 (or 1) over two Q of its own
        a[2 * g + 1] = ((0 if holds[g] else 1) - a[2 * g] * pool[2 * g]) * pow(pool[2 * g + 1], -1, R) % R
    g1, g2 = points(eng, oracle, a, list(range(8)), pool)
    (bits, delta), rec = launches(eng, lambda: run(eng, g1, g2, offsets_u64(sizes)), MILLER_KERNELS)
    assert bits == holds
    assert delta == stats(exact=4, equations=0, exact_calls=1)
    assert set(rec) <= set(VARIABLE_Q), rec


# ---------------------------------------------------------------- 6. offsets that do not start at 0
def test_offsets_need_not_start_at_zero(eng, oracle):
    sizes = [1, 0, 2, 3, 0, 2, 0]                                       # the first pair belongs to no equation
    holds = [False, True, True, False, True, True, True]
    g1, g2, actual = batch(eng, oracle, 6, sizes, holds)
    g1 = bytes([g1[0] ^ 1]) + g1[1:]                                    # ... and is no point at all
    off = offsets_u64(sizes)[1:]
    bits, delta = run(eng, g1, g2, off)
    assert bits == actual[1:] == [True, True, False, True, True, True]
    # 7 pairs over at most 3 Q: one segment only, so every equation -- the empty ones at both ends are eligible -- goes to the exact
    # call, whose offsets are the caller's from equation 0 on
    assert delta == stats(exact=6)


# ---------------------------------------------------------------- 7. segments on an engine of small launches
def test_segments_with_one_false_equation(M, oracle, monkeypatch, eng):
    n_eq = 24
    holds = [g != n_eq - 2 for g in range(n_eq)]                        # in the last of the 4 segments of 6 equations
    g1, g2, actual = batch(eng, oracle, 7, [3] * n_eq, holds)
    off = offsets_u64([3] * n_eq)
    e = fresh_engine(M, monkeypatch, "64")                              # 72 pairs: the exact call runs two launches
    try:
        e.set_pairing_check_rlc_segments(4)
        bits, delta = run(e, g1, g2, off)
        assert bits == actual == holds
        assert delta == stats(round2=18, exact=6, equations=5, failed=1)
        e.set_pairing_check_rlc_segments(1)                             # no second round: every eligible equation to the exact call
        bits, delta = run(e, g1, g2, off)
        assert bits == holds and delta == stats(exact=n_eq)
        e.set_pairing_check_rlc_segments(0)                             # the default rule: min(256, 72 / 6) = 12 segments of 2
        bits, delta = run(e, g1, g2, off)
        assert bits == holds and delta == stats(round2=22, exact=2, equations=13, failed=1)
    finally:
        e.close()


# ---------------------------------------------------------------- 8. seed = None, argument errors
def test_seed_from_the_os_and_argument_errors(eng, oracle):
    g1b, g2b, actual = batch(eng, oracle, 8, [2] * 6, [True, True, False, True, True, True])
    bits, delta = run(eng, g1b, g2b, offsets_u64([2] * 6), None)
    assert bits == actual and delta["round1_equations"] == 0 and delta["exact_equations"] >= 1
    lib, ctx = eng._lib, eng._ctx
    u8 = ctypes.POINTER(ctypes.c_uint8); u64 = ctypes.POINTER(ctypes.c_uint64)
    g1 = np.frombuffer(oracle.g1_generator() * 4, dtype=np.uint8); g2 = np.frombuffer(oracle.g2_generator() * 4, dtype=np.uint8)
    sd = np.frombuffer(SEED, dtype=np.uint8)
    out = np.zeros(8, dtype=np.uint8)
    p1, p2, po, ps = g1.ctypes.data_as(u8), g2.ctypes.data_as(u8), out.ctypes.data_as(u8), sd.ctypes.data_as(u8)
    fn = lib.blsbn254_pairing_check_batch_rlc

    def call(off, n, a=p1, b=p2, o=po, seed=ps, c=ctx):
        arr = np.ascontiguousarray(np.asarray(off, dtype=np.uint64))
        return fn(c, a, b, arr.ctypes.data_as(u64) if len(off) else None, ctypes.c_size_t(n), seed, o)

    assert call([0, 3, 1], 2) == E_ARG                               # decreasing offsets
    assert call([0, (1 << 23) + 1], 1) == E_ARG                      # more than 2^23 pairs
    assert call([0, 2], 1, a=None) == E_ARG
    assert call([0, 2], 1, b=None) == E_ARG
    assert call([0, 2], 1, o=None) == E_ARG
    assert call([], 1) == E_ARG                                      # no offsets
    assert call([0, 2], 1, c=None) == E_ARG
    assert call([0], 0) == 0 and call([], 0, a=None, b=None, o=None, seed=None) == 0
    assert call([0, 2, 4], 2) == 0 and out[0] == 0                   # e(G1, G2)^2 != 1
    assert call([0, 2, 4], 2, seed=None) == 0 and out[0] == 0
    assert lib.blsbn254_pairing_check_rlc_stats(ctx, None) == E_ARG
    assert lib.blsbn254_pairing_check_rlc_stats(None, (ctypes.c_uint64 * 8)()) == E_ARG
    assert lib.blsbn254_set_pairing_check_rlc_segments(ctx, ctypes.c_size_t(4097)) == E_ARG
    assert lib.blsbn254_set_pairing_check_rlc_segments(None, ctypes.c_size_t(4)) == E_ARG
    eng.set_pairing_check_rlc_segments(4096)
    eng.set_pairing_check_rlc_segments(0)
    assert eng.pairing_check_batch_rlc(b"", b"", [0]) == b""
    s0 = eng.pairing_check_rlc_stats()
    assert eng.pairing_check_batch_rlc(b"", b"", [0, 0, 0]) == b"\x03"   # empty equations only: they hold, as in the exact call
    s1 = eng.pairing_check_rlc_stats()
    assert {k: s1[k] - s0[k] for k in PCR_STATS} == stats(exact=2, equations=0, exact_calls=1)
    with pytest.raises(ValueError):
        eng.pairing_check_batch_rlc(b"", b"", [])


# ---------------------------------------------------------------- 9. a sequence on one context
def test_sequence_on_one_context(eng, M, oracle):
    """the RLC call with a false equation, the aggregate verify by random linear combination, the exact pairing check, the RLC call
    again under another seed: each result equals the same call on a context of its own"""
    dst = M.DEFAULT_DST
    holds = [g != 3 for g in range(10)]
    g1, g2, _ = batch(eng, oracle, 9, [2] * 10, holds)
    off = offsets_u64([2] * 10)
    D = Data(eng, [3] * 10, dst, salt=12)
    D.flip_message(4)
    keys, msgs, sigs, _ = D.args()
    calls = [lambda e: e.pairing_check_batch_rlc(g1, g2, off, SEED),
             lambda e: e.aggregate_verify_batch_rlc(keys, msgs, sigs, dst, SEED),
             lambda e: e.pairing_check_batch(g1, g2, off),
             lambda e: e.pairing_check_batch_rlc(g1, g2, off, SEED_B)]
    want = []
    for f in calls:
        fresh = M.Engine(0)
        try:
            want.append(f(fresh))
        finally:
            fresh.close()
    assert bits_of(want[0], 10) == bits_of(want[2], 10) == bits_of(want[3], 10) == holds
    assert bits_of(want[1], 10) == [g != 4 for g in range(10)]
    e = M.Engine(0)
    try:
        assert [f(e) for f in calls] == want
        assert e.pairing_check_rlc_stats()["calls"] == 2 and e.aggregate_rlc_stats()["calls"] == 1
    finally:
        e.close()
