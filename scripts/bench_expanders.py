"""What a message expander other than the default costs: n = 262 144 tuples with 32-byte messages over a pool of 1024 keys, signed
and verified under each expander id (blsbn254_set_expander) on ONE context, the ids interleaved round by round in one process.
Per id: the wall time of verify_batch (host clock around a call that ends synchronised) and, from the engine's HIP-event profile
in passes of their own, the time of the hash-to-G1 launch of that call -- the homogeneous form (mode 3) of k_hash_to_g1 under id 0
and of k_hash_to_g1_x under the others.  The yardstick is id 0, the XMD-SHA-256 kernel the parent commit has, measured in the
same run: every figure is also given as a ratio to it.  Every bitmap must be all ones, and all zero under another id.
Usage: python scripts/bench_expanders.py [--out profiles/expanders.json] [--n 262144] [--reps 7] -> JSON"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import blsbn254_loader; M = blsbn254_loader.load()
from tests import synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join("profiles", "expanders.json"))
ap.add_argument("--n", type=int, default=262144)
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
N, POOL, REPS, WARM, PROF = args.n, 1024, max(args.reps, 1), 2, 5
NAMES = {M.EXPAND_XMD_SHA256: "xmd_sha256", M.EXPAND_XMD_KECCAK256: "xmd_keccak256", M.EXPAND_XMD_SHA3_256: "xmd_sha3_256",
         M.EXPAND_XOF_SHAKE128: "xof_shake128", M.EXPAND_XOF_SHAKE256: "xof_shake256"}
dst = M.DEFAULT_DST
e = M.Engine(0)
pool = min(POOL, N)
skb = b"".join(synth.sk_of(k).to_bytes(32, "big") for k in range(pool))
pk_pool = e.sk_to_pk_batch(skb, pool)
pks = pk_pool * (N // pool) + pk_pool[:128 * (N % pool)]
sk_all = skb * (N // pool) + skb[:32 * (N % pool)]
msgs = [synth.msg_of(i) for i in range(N)]
ones = synth.bitmap_of([True] * N)
sigs = {}
for xid in NAMES:
    e.set_expander(xid)
    sigs[xid] = e.sign_batch(sk_all, msgs, dst)
    assert e.verify_batch(pks, msgs, sigs[xid], dst) == ones, NAMES[xid]
e.set_expander(M.EXPAND_XMD_SHA256)
assert e.verify_batch(pks[:128 * 4096], msgs[:4096], sigs[M.EXPAND_XMD_KECCAK256][:64 * 4096], dst) == bytes(512)     # Keccak signatures under SHA-256


def stats(v):
    a = np.sort(np.array(v))
    return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a[0]), 4), "max_ms": round(float(a[-1]), 4), "reps": len(v)}


def verify(xid):
    e.set_expander(xid)                                  # outside the timed region
    t = time.perf_counter()
    bm = e.verify_batch(pks, msgs, sigs[xid], dst)
    ms = (time.perf_counter() - t) * 1e3
    assert bm == ones, NAMES[xid]
    return ms


wall = {xid: [] for xid in NAMES}
for r in range(WARM + REPS):
    for xid in NAMES:
        ms = verify(xid)
        if r >= WARM:
            wall[xid].append(ms)
hash_ms, launches = {xid: [] for xid in NAMES}, {}
e.profile_enable(True)
for _ in range(PROF):
    for xid in NAMES:
        e.profile_reset()
        verify(xid)
        rec = e.profile_read()["hash_to_g1"]
        hash_ms[xid].append(rec["total_ms"]); launches[xid] = rec["launches"]
e.profile_enable(False); e.profile_reset()
e.close()
base_w, base_h = np.median(wall[0]), np.median(hash_ms[0])
out = {"method": "one context, one process, the expander ids interleaved round by round; verify_batch: host clock around the call (host pointers, ends "
                 "synchronised), %d warm-up + %d timed rounds; hash_to_g1: the HIP-event profile's total for the hash-to-G1 launches of one verify_batch "
                 "(homogeneous output, mode 3), %d further rounds; ratios are medians over the median of id 0 (XMD-SHA-256, the parent commit's "
                 "kernel) of the same run" % (WARM, REPS, PROF),
       "n": N, "keys": pool, "message_bytes": 32, "dst_bytes": len(dst), "ids": {}}
for xid, name in NAMES.items():
    row = {"id": xid, "verify_batch": stats(wall[xid]), "hash_to_g1": dict(stats(hash_ms[xid]), launches=launches[xid])}
    row["verify_batch"]["over_sha256"] = round(float(np.median(wall[xid]) / base_w), 3)
    row["hash_to_g1"]["over_sha256"] = round(float(np.median(hash_ms[xid]) / base_h), 3)
    out["ids"][name] = row
os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
open(args.out, "w").write(json.dumps(out, indent=1) + "\n")
print(json.dumps(out, indent=1))
