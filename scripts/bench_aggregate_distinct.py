"""What the distinct-message rule costs on the device, and what a caller pays for the weaker check on the host today:
    python scripts/bench_aggregate_distinct.py --out profiles/aggregate_distinct.json
Shapes 2^16 x 4, 2^18 x 1 and 2^10 x 4 (groups x pairs per group) over the 1024-key pool, all groups honest and all messages
distinct (32 bytes each), on one GPU.  The forms are interleaved round by round in one process, two warm-up rounds and --reps (7)
timed ones, host clock around the synchronous call through Engine; reported: the median with min .. max.
  1. the new calls against their parents on the same input: aggregate_verify_batch_distinct / aggregate_verify_batch, and the
     _rlc pair (seed = None, the production setting); hash_distinct_batch alone.  The stage's kernel time (k_md_keys + k_md_insert,
     the engine's HIP-event profile of seven further rounds) and its share of the new call's median; for the RLC form k_md_keys
     normalises the homogeneous points (one inversion per pair), so its time beside the affine form's k_md_keys is that cost.
  2. the new call against what a caller does today: the parent call plus a per-group set of the message BYTES on the host, in
     plain Python (one set per group) and in numpy (the 32-byte messages as four words each, every two pairs of a group compared
     across all groups at once -- which needs messages of one length and small groups of one size, as this input has; the join
     of the message list into one buffer is part of the time, as it is part of the call's).  The composition is
     the sum of the two times of the same round.  The host check sees bytes only: under the try-and-increment maps it is the
     weaker check, whatever it costs."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POOL, WARM, PROF = 1024, 2, 7


def stats(v):
    a = np.sort(np.array(v, dtype=np.float64))
    return {"median_ms": round(float(np.median(a)), 3), "min_ms": round(float(a[0]), 3), "max_ms": round(float(a[-1]), 3), "reps": len(v)}


def python_check(msgs, n_g, k):
    return [len(set(msgs[k * g:k * g + k])) != k for g in range(n_g)]


def numpy_check(msgs, n_g, k):
    w = np.frombuffer(b"".join(msgs), dtype=np.uint64).reshape(n_g, k, 4)
    rep = np.zeros(n_g, dtype=bool)
    for i in range(k):
        for j in range(i + 1, k):
            rep |= (w[:, i] == w[:, j]).all(axis=1)
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "aggregate_distinct.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="16x4,18x1,10x4", help="log2(groups) x pairs per group")
    a = ap.parse_args()
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
    pks, sigs = bytes(pks), bytes(sigs)
    rows = []
    for lg, k in shapes:
        n_g = 1 << lg
        N = n_g * k
        goff = np.arange(0, N + 1, k, dtype=np.uint64)
        gp, gm = pks[:128 * N], list(msgs[:N])
        ga = sigs[:64 * N] if k == 1 else b"".join(O.aggregate_sigs(sigs[64 * k * g:64 * k * (g + 1)], k) for g in range(n_g))
        ones, zeros = np.packbits(np.ones(n_g, dtype=np.uint8), bitorder="little").tobytes(), bytes((n_g + 7) // 8)
        forms = {
            "exact": lambda: eng.aggregate_verify_batch_flat(gp, gm, goff, ga, dst),
            "exact_distinct": lambda: eng.aggregate_verify_batch_distinct_flat(gp, gm, goff, ga, dst),
            "rlc": lambda: eng.aggregate_verify_batch_rlc_flat(gp, gm, goff, ga, dst),
            "rlc_distinct": lambda: eng.aggregate_verify_batch_rlc_distinct_flat(gp, gm, goff, ga, dst),
            "hash_distinct": lambda: eng.hash_distinct_batch(gm, goff, dst),
            "host_check_python": lambda: python_check(gm, n_g, k),
            "host_check_numpy": lambda: numpy_check(gm, n_g, k),
        }
        assert forms["exact"]() == ones and forms["rlc"]() == ones
        assert forms["exact_distinct"]() == (ones, zeros) and forms["rlc_distinct"]() == (ones, zeros) and forms["hash_distinct"]() == zeros
        assert not any(forms["host_check_python"]()) and not forms["host_check_numpy"]().any()
        ms = {f: [] for f in forms}
        for r in range(WARM + a.reps):
            for f, fn in forms.items():
                t0 = time.perf_counter(); fn(); dt = 1e3 * (time.perf_counter() - t0)
                if r >= WARM:
                    ms[f].append(dt)
        for parent in ("exact", "rlc"):
            for host in ("python", "numpy"):
                ms["%s_plus_%s" % (parent, host)] = [x + y for x, y in zip(ms[parent], ms["host_check_" + host])]
        kern = {f: {"md_keys": [], "md_insert": []} for f in ("exact_distinct", "rlc_distinct", "hash_distinct")}
        eng.profile_enable(True)
        for _ in range(PROF):
            for f in kern:
                eng.profile_reset()
                forms[f]()
                rec = eng.profile_read()
                for name in kern[f]:
                    kern[f][name].append(rec[name]["total_ms"])
        eng.profile_enable(False); eng.profile_reset()
        med = lambda f: float(np.median(ms[f]))
        row = {"log2_groups": lg, "groups": n_g, "pairs_per_group": k, "pairs": N, "distinct_keys": min(POOL, N), "message_bytes": 32,
               "slots": eng.msg_distinct_stats()["slots"], "call_ms": {f: stats(v) for f, v in ms.items()}, "stage_kernels_ms": {}}
        for f in kern:
            stage = float(np.median(kern[f]["md_keys"]) + np.median(kern[f]["md_insert"]))
            row["stage_kernels_ms"][f] = {"md_keys": stats(kern[f]["md_keys"]), "md_insert": stats(kern[f]["md_insert"]), "stage_median_ms": round(stage, 3),
                                          "share_of_call": round(stage / med(f), 4)}
        row["normalisation_ms"] = round(float(np.median(kern["rlc_distinct"]["md_keys"]) - np.median(kern["exact_distinct"]["md_keys"])), 3)
        row["ratios"] = {"exact_distinct_over_exact": round(med("exact_distinct") / med("exact"), 4),
                         "rlc_distinct_over_rlc": round(med("rlc_distinct") / med("rlc"), 4)}
        for parent in ("exact", "rlc"):
            for host in ("python", "numpy"):
                row["ratios"]["%s_distinct_over_%s_plus_%s" % (parent, parent, host)] = round(med(parent + "_distinct") / med("%s_plus_%s" % (parent, host)), 4)
            for host in ("python", "numpy"):
                extra = med(parent + "_distinct") - med(parent)
                row["ratios"]["%s_stage_cost_over_%s_check" % (parent, host)] = round(extra / med("host_check_" + host), 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
    eng.close()
    out = {"method": "one process, one context; the forms interleaved round by round, %d warm-up + %d timed rounds, host clock around the synchronous call "
                     "through Engine; median with min .. max; kernel times: the engine's HIP-event profile, %d further rounds; compositions: the sum of the "
                     "two times of the same round; *_stage_cost_over_*_check: (median of the new call - median of its parent) / median of the host check"
                     % (WARM, a.reps, PROF),
           "pool": POOL, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
