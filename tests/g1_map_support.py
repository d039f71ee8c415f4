"""The model the tests of blsbn254_set_g1_map compare against: the try-and-increment map to G1 of the EVM's BN254 BLS contracts,
in pure Python and written twice -- once as the contracts' loop (Euler's criterion, pow(beta, (p + 1) // 4, p)), once as a
property any result must have (on the curve, y equal to that power, every skipped x a non-residue, k the number skipped) -- and
helpers that find digests with a prescribed run of skipped candidates, which is cheap under TAI_DIGEST because x0 IS the input.
The plain digests come from hashlib and, for Keccak-256, from tests/expander_support.py (pinned by tests/test_expander_model.py).
tests/test_g1_map_model.py checks the two formulations against each other before any other test relies on this file.  CPU only.
No vector from a deployed contract is available to this repository: the map is pinned by construction."""
import functools
import hashlib

from oracle.pyref import bn254 as ref
from tests import expander_support as X

P = ref.P
SVDW, TAI_DIGEST, TAI_HASH = range(3)
MAPS = (SVDW, TAI_DIGEST, TAI_HASH)
CAP = 65536                                   # TAI_CAP of the library (lane_hash_tai.h)

PLAIN = {X.XMD_SHA256: lambda m: hashlib.sha256(m).digest(), X.XMD_KECCAK256: X.keccak256, X.XMD_SHA3_256: lambda m: hashlib.sha3_256(m).digest(),
         X.XOF_SHAKE128: lambda m: hashlib.shake_128(m).digest(32), X.XOF_SHAKE256: lambda m: hashlib.shake_256(m).digest(32)}


def x0_of(map_id, xid, msg):
    """the start of the search: the message (TAI_DIGEST) or its plain digest under the expander's hash (TAI_HASH), as one
    big-endian integer mod p"""
    assert map_id in (TAI_DIGEST, TAI_HASH)
    return int.from_bytes(msg if map_id == TAI_DIGEST else PLAIN[xid](msg), "big") % P


def is_residue(x):
    """Euler's criterion on beta = x^3 + 3 (never 0: -3 is not a cube mod p, tests/test_g1_map_model.py)"""
    return pow((x * x * x + 3) % P, (P - 1) // 2, P) == 1


def contract_loop(x0, cap=CAP):
    """the contracts' loop: ((x, y), k) with k the candidates skipped, or (None, cap) when `cap` candidates were non-residues"""
    x = x0 % P
    for k in range(cap):
        beta = (x * x * x + 3) % P
        if pow(beta, (P - 1) // 2, P) == 1:
            return (x, pow(beta, (P + 1) // 4, P)), k
        x = (x + 1) % P
    return None, cap


def holds(x0, pt, k):
    """the same map as a property of a claimed result"""
    x, y = pt
    beta = (x * x * x + 3) % P
    return (x == (x0 + k) % P and y * y % P == beta and y == pow(beta, (P + 1) // 4, P)
            and all(not is_residue((x0 + j) % P) for j in range(k)))


def run_of(x0):
    """candidates the search skips from x0"""
    return contract_loop(x0)[1]


def point_bytes(pt):
    """64 bytes x || y; a search that hit the cap yields the off-curve (0, 0)"""
    x, y = pt if pt is not None else (0, 0)
    return x.to_bytes(32, "big") + y.to_bytes(32, "big")


def hash_to_g1(map_id, xid, msg, cap=CAP):
    return contract_loop(x0_of(map_id, xid, msg), cap)[0]


def hash_bytes(map_id, xid, msg, cap=CAP):
    return point_bytes(hash_to_g1(map_id, xid, msg, cap))


def sign(map_id, xid, sk, msg):
    return ref.g1_mul(hash_to_g1(map_id, xid, msg), sk % ref.R)


# ---- digests with a prescribed run
WINDOW = 0x1f3a << 232                        # where the scan starts: any fixed value below p - 2^20 serves


@functools.lru_cache(maxsize=None)
def _runs(count_long, long_run):
    """run lengths of consecutive x from WINDOW on: scanned in pieces until `count_long` starts with a run >= long_run were seen.
    Returns (base, runs) with runs[i] = run_of(base + i), None for the last few whose run is still open."""
    res = []
    while True:
        lo = len(res)
        res.extend(is_residue(WINDOW + i) for i in range(lo, lo + 8192))
        runs, r = [0] * len(res), None
        for i in range(len(res) - 1, -1, -1):
            r = 0 if res[i] else (None if r is None else r + 1)
            runs[i] = r
        closed = [v for v in runs if v is not None]
        if sum(1 for v in closed if v >= long_run) >= count_long:
            return WINDOW, runs


def digests_with_run(run, count, at_least=False, skip=0):
    """`count` distinct 32-byte digests whose search skips exactly `run` candidates (at_least: `run` or more), from the scanned
    window, after passing over the first `skip` such; each is checked against the model's own run length"""
    base, runs = _runs(4, 12)
    hits = [base + i for i, v in enumerate(runs) if v is not None and (v >= run if at_least else v == run)]
    assert len(hits) >= skip + count, (run, count, len(hits))
    out = hits[skip:skip + count]
    for x0 in out:
        got = run_of(x0)
        assert got >= run if at_least else got == run, (x0, got, run)
    return [x.to_bytes(32, "big") for x in out]


# the digests whose reduction mod p matters: p - 1 (the search wraps to 0 if it is skipped), p, p + 5, 2^256 - 1
EDGE_DIGESTS = [v.to_bytes(32, "big") for v in (P - 1, P, P + 5, (1 << 256) - 1)]
# ... and messages of other lengths under TAI_DIGEST: empty, 1, 31, 33 and 100 bytes
ODD_LENGTHS = [b"", b"\x07", bytes(range(1, 32)), bytes(range(200, 233)), bytes((7 * i + 1) & 0xff for i in range(100))]
assert [len(m) for m in ODD_LENGTHS] == [0, 1, 31, 33, 100]


def mixed_wave(n, seed=0):
    """n digests for one launch whose waves mix short and long searches: runs of 0, 1, 2, 3 and 5 mixed, the edge digests, and in
    every wave of 64 one lane with a run of at least 12 (the condition is the model's own run length, asserted above)"""
    each = n // 5 + 1
    per = {r: digests_with_run(r, each, skip=seed * each) for r in (0, 1, 2, 3, 5)}
    long_ones = digests_with_run(12, (n + 63) // 64, at_least=True, skip=seed % 4)
    out = []
    for i in range(n):
        out.append(per[(0, 1, 2, 3, 5)[i % 5]][i // 5])
    for w in range((n + 63) // 64):
        out[min(64 * w + 37, n - 1)] = long_ones[w]
    for j, d in enumerate(EDGE_DIGESTS):
        if 2 + 9 * j < n and (2 + 9 * j) % 64 != 37:
            out[2 + 9 * j] = d
    return out
