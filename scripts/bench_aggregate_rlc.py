"""Aggregate verify over groups by random linear combination (blsbn254_aggregate_verify_batch_rlc) against the exact call
(blsbn254_aggregate_verify_batch, unchanged by the RLC work: its time IS the parent commit's) on one GPU, both in the same run:
    python scripts/bench_aggregate_rlc.py --out profiles/aggregate_rlc.json
Every row of DESIGN.md 6e (2^10 x 4, 2^14 x 4, 2^16 x 4, 2^18 x 1, 2^12 x 64 over the 1024-key pool) and 16 x 4, each three ways: all
honest, one wrong message in every 4096th group, one in every 16th.  Call time through Engine (seed = None, the production
setting), host clock around the synchronous call, min of --reps repetitions after one warm-up, max - min recorded as the spread;
the bitmap of both calls is checked against the pattern before anything is timed.  Per-kernel times of the RLC call come from the
engine's HIP-event profile of one further call.  On the 1-in-4096 rows the cap S_max of the default rule S = min(S_max, N / (2 u))
is tried at 16, 64 and 256 (blsbn254_set_aggregate_rlc_segments with the S that cap gives); all three times are recorded."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POOL = 1024
S_MAX_TRIED = (16, 64, 256)
KERNELS = ("hash_to_g1", "g2_prepare", "agr_group", "agr_weigh", "g1_seg_sum", "miller_wide_1p", "miller_tri_1p", "miller_hpk1p", "miller_hpk2p", "miller_hpk2r",
           "fp12_seg_prod", "fe_easy", "fe_hard_wide", "fe_tri_hard", "fe_expx_h1", "fe_expx_h2", "fe_expx", "fe_h3")


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return round(1e3 * min(ts), 3), round(1e3 * (max(ts) - min(ts)), 3)


def groups_of(O, batch, n_g, k, every):
    """the first n_g * k tuples as n_g groups of k: flat keys, message list, aggregate signatures, expected bitmap, bad groups;
    every: group g with g mod every == every - 1 has one message flipped (0: none)"""
    pks, msgs, sigs = batch
    n = n_g * k
    msgs = list(msgs[:n])
    aggs = sigs[:64 * n] if k == 1 else b"".join(O.aggregate_sigs(sigs[64 * k * g:64 * k * (g + 1)], k) for g in range(n_g))
    want = np.ones(n_g, dtype=np.uint8)
    bad = list(range(every - 1, n_g, every)) if every else []
    for g in bad:
        i = k * g + (g // every) % k
        msgs[i] = bytes([msgs[i][0] ^ 1]) + msgs[i][1:]
        want[g] = 0
    return pks[:128 * n], msgs, aggs, np.packbits(want, bitorder="little").tobytes(), len(bad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="10x4,14x4,16x4,18x1,12x64,4x4", help="log2(groups) x pairs per group")
    a = ap.parse_args()
    assert a.reps >= 5, "at least 5 repetitions"
    import blsbn254_loader
    M = blsbn254_loader.load()
    from oracle import oracle as O
    from tests import synth
    O.build()
    eng = M.Engine(0)
    dst = M.DEFAULT_DST
    shapes = [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",")]
    n_max = max((1 << lg) * k for lg, k in shapes)
    pks, msgs, sigs, _ = synth.make_batch_gpu(eng, O, n_max, dst, pool=POOL, invalid_every=0, spot=16)
    batch = (bytes(pks), msgs, bytes(sigs))
    rows = []
    for lg, k in shapes:
        n_g = 1 << lg
        N, u = n_g * k, min(POOL, n_g * k)
        goff = np.arange(0, N + 1, k, dtype=np.uint64)
        for mode, every in (("honest", 0), ("1_in_4096", 4096), ("1_in_16", 16)):
            gp, gm, ga, want, n_bad = groups_of(O, batch, n_g, k, every)
            rlc = lambda: eng.aggregate_verify_batch_rlc_flat(gp, gm, goff, ga, dst)
            exact = lambda: eng.aggregate_verify_batch_flat(gp, gm, goff, ga, dst)
            eng.set_aggregate_rlc_segments(0)
            assert exact() == want, "the exact bitmap differs from the pattern"
            s0 = eng.aggregate_rlc_stats()
            assert rlc() == want, "the RLC bitmap differs from the pattern"
            s1 = eng.aggregate_rlc_stats()
            row = {"log2_groups": lg, "groups": n_g, "pairs_per_group": k, "pairs": N, "distinct_keys": u, "mode": mode, "bad_groups": n_bad,
                   "stats_of_one_call": {x: s1[x] - s0[x] for x in s1}}
            te, se = timed(exact, a.reps)
            tr, sr = timed(rlc, a.reps)
            eng.profile_reset(); eng.profile_enable(True)
            rlc()
            eng.profile_enable(False)
            prof = eng.profile_read()
            eng.profile_reset()
            row.update({"exact_ms": te, "exact_spread_ms": se, "rlc_ms": tr, "rlc_spread_ms": sr, "rlc_over_exact": round(tr / te, 3),
                        "rlc_below_exact_beyond_spreads": bool(te - tr > se + sr),
                        "rlc_kernels_ms": {x: {"launches": prof[x]["launches"], "ms": round(prof[x]["total_ms"], 3)} for x in KERNELS if x in prof},
                        "rlc_kernel_total_ms": round(sum(v["total_ms"] for v in prof.values()), 3)})
            if mode == "1_in_4096" and n_bad:
                tried = {}
                for s_max in S_MAX_TRIED:
                    S = min(s_max, N // (2 * u), n_g)
                    eng.set_aggregate_rlc_segments(S if S >= 2 else 1)
                    assert rlc() == want
                    t, sp = timed(rlc, a.reps)
                    tried[str(s_max)] = {"segments": S, "rlc_ms": t, "rlc_spread_ms": sp}
                eng.set_aggregate_rlc_segments(0)
                row["s_max_tried"] = tried
            print(json.dumps(row), flush=True)
            rows.append(row)
    stats = eng.aggregate_rlc_stats()
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"timing": "host clock around the synchronous call through Engine, min of reps after one warm-up; spread = max - min of the reps; "
                                 "both calls in the same run, the exact call first",
                       "exact": "blsbn254_aggregate_verify_batch, unchanged by the RLC call: the parent commit's number",
                       "reps": a.reps, "pool": POOL, "s_max_tried": list(S_MAX_TRIED), "rows": rows, "stats": stats}, f, indent=1)


if __name__ == "__main__":
    main()
