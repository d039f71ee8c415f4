"""Latency of ONE small call, where the host side shows: verify_batch of 64 tuples over 4 keys through the host-pointer C ABI,
wall time over repeated calls, with the launch record's kernel-time sum of further calls beside it.  A fresh process per
measurement; BLSBN254_LIB selects another build of the library (a parent commit's, for an A/B of host-side changes).
Usage: python scripts/bench_verify_latency.py [calls]  ->  one JSON line on stdout"""
import json, os, statistics, sys, time
sys.path.insert(0, os.getcwd())
import blsbn254_loader; M = blsbn254_loader.load()
from oracle import oracle as O
from tests import synth

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 300
dst, n = M.DEFAULT_DST, 64
pks, msgs, sigs, exp = synth.make_batch(O, n, dst, pool=4, invalid_every=7, uniq=16)
want = synth.bitmap_of(exp)
e = M.Engine(0)
for _ in range(30):                                     # workspaces reserved, the store of prepared keys filled, clocks up
    assert e.verify_batch(pks, msgs, sigs, dst) == want
wall = []
for _ in range(calls):
    t = time.perf_counter()
    e.verify_batch(pks, msgs, sigs, dst)
    wall.append((time.perf_counter() - t) * 1e3)
e.profile_enable(True); e.profile_reset()
reps = 50
for _ in range(reps):
    e.verify_batch(pks, msgs, sigs, dst)
rec = e.profile_read(); e.profile_enable(False)
e.close()
print(json.dumps({"n": n, "calls": calls, "wall_ms_median": round(statistics.median(wall), 4), "wall_ms_mean": round(statistics.fmean(wall), 4),
                  "wall_ms_min": round(min(wall), 4), "kernel_ms_sum": round(sum(v["total_ms"] for v in rec.values()) / reps, 4),
                  "launches_per_call": sum(v["launches"] for v in rec.values()) // reps, "lib": os.environ.get("BLSBN254_LIB", "built")}))
