"""What the tests of the pairing-product checks over ragged groups by random linear combination share: the Python models of the
weight derivation and of the plan (bls-bn254_amd/csrc/pairing_check_rlc.h, pairing_check_rlc_plan.h over aggregate_rlc_plan.h), the
names the feature adds, the oracle's composition of a pair's and an equation's validity, and the builders of closed-form equations
(P = [a] G1gen, Q = [b] G2gen with b from a small pool: the equation holds iff sum a_j b_j = 0 mod r) the GPU tests run it on."""
import hashlib

from tests import synth
from tests.aggregate_rlc_support import cut, failed_ranges, segments, weight_of_digest  # noqa: F401 (the plan the two calls share)
from tests.helpers import IDENT1, IDENT2, b32

PCR_KERNELS = ("k_pcr_pairs", "k_pcr_eq", "k_pcr_weigh", "k_pcr_items")
PCR_SYMBOLS = ("blsbn254_pairing_check_batch_rlc", "blsbn254_set_pairing_check_rlc_segments", "blsbn254_pairing_check_rlc_stats")
PCR_STATS = ("calls", "round1_equations", "round2_equations", "exact_equations", "ineligible_equations", "equations", "exact_calls", "failed_segments")
S_MAX = 256                                                             # pairing_check_rlc_plan.h PCR_SMAX
MERGE_GAP = 1 << 15                                                     # pairing_check_rlc_plan.h PCR_MERGE_GAP
MAX_KEYS = 1 << 16                                                      # host_common.h PREP_MAX_KEYS
MAX_SEGMENTS = 4096                                                     # aggregate_rlc_plan.h AGR_MAX_SEGMENTS
SEED = bytes(range(101, 133))
R = synth.R


def weight(seed, g):
    """(a_g, b_g): r_g = a_g + b_g lambda"""
    return weight_of_digest(hashlib.sha256(seed + b"PCRLC" + g.to_bytes(8, "little")).digest())


def round1(N, u, max_keys=MAX_KEYS):
    return N != 0 and u * 2 <= N and u <= max_keys


def g1_is_identity(p):
    return p[:32] == bytes(32)


def g2_is_identity(q):
    return q[:64] == bytes(64)


def pair_truth(oracle, p, q):
    """(ok, skip) of one pair from the oracle's checks, composed as the exact call's tests compose them: P decodes and is the
    identity or on the curve, Q decodes and is the identity or on the curve and in the r-torsion; skipped with an identity member"""
    P = synth.P
    coords = [int.from_bytes(p[i:i + 32], "big") for i in (0, 32)] + [int.from_bytes(q[i:i + 32], "big") for i in (0, 32, 64, 96)]
    id1, id2 = g1_is_identity(p), g2_is_identity(q)
    dec1 = coords[0] < P and (id1 or coords[1] < P)
    dec2 = coords[2] < P and coords[3] < P and (id2 or (coords[4] < P and coords[5] < P))
    ok1 = dec1 and (id1 or bool(oracle.g1_check_batch(p, 1)[0] & 1))
    ok2 = dec2 and (id2 or bool(oracle.g2_check_batch(q, 1)[0] & 1))
    return ok1 and ok2, id1 or id2


def plan(setting, N, u, G, passed1, elig, off, passed2=None):
    """The model of a call that takes round 1: (S of round 2 or 1, the ranges of the exact sub-calls, equations sent to them).
    passed2: the is-one bytes of round 2's segments when it runs."""
    if passed1:
        return 1, [], 0
    S = segments(setting, N, u, G, S_MAX)
    bound, passed = (cut(G, S)[0], passed2) if S >= 2 else ([0, G], [0])
    n, ranges = failed_ranges(bound, passed, elig, off, MERGE_GAP)
    return S, ranges, n


def closed_form(rnd, sizes, holds, pool, zero=()):
    """(a per pair, pool index per pair, whether each equation holds): equation g's sum a_j pool[k_j] is 0 mod r when holds[g]
    (else 1).  Pairs listed in `zero` (indices within the call) get a = 0 (an identity P); the last pair with a non-zero a
    absorbs the sum, and an equation without one holds whatever holds[g] says."""
    a, kk, actual = [], [], []
    zero = set(zero)
    pos = 0
    for g, n in enumerate(sizes):
        ag = [0 if pos + j in zero else rnd.randrange(1, R) for j in range(n)]
        kg = [rnd.randrange(len(pool)) for _ in range(n)]
        nz = [j for j in range(n) if ag[j]]
        if nz:
            last = nz[-1]
            rest = sum(ag[j] * pool[kg[j]] for j in range(n) if j != last) % R
            ag[last] = ((0 if holds[g] else 1) - rest) * pow(pool[kg[last]], -1, R) % R
            if ag[last] == 0:                                          # (one chance in r)
                raise ValueError("degenerate closed form; use another seed")
        a += ag; kk += kg; pos += n
        actual.append(bool(holds[g]) if nz else True)
    return a, kk, actual


def points(eng, oracle, a, kk, pool):
    """the encodings: P_j = [a_j] G1gen through the engine (a = 0: the identity), Q_j = [pool[k_j]] G2gen through the oracle"""
    n = len(a)
    if n == 0:
        return b"", b""
    P = bytearray(eng.g1_mul_batch(oracle.g1_generator() * n, b"".join(map(b32, a)), n))
    for j, v in enumerate(a):
        if v == 0:
            P[64 * j:64 * j + 64] = IDENT1
    qs = [oracle.g2_mul(oracle.g2_generator(), b) if b else IDENT2 for b in pool]
    return bytes(P), b"".join(qs[k] for k in kk)
