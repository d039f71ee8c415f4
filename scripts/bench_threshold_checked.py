"""The checked threshold combine (blsbn254_threshold_combine_checked_batch) on one GPU against the composition the other entry
points offer for the same job, in the same build and on the same inputs: threshold_verify_shares_batch -> the first t live
shares of every group picked on the host -> threshold_combine_batch.  Groups of 7 shares with t = 5 and ids 1 .. 7; one run
with every partial good, one with one bad candidate (signed over another message) among the first t in every 16th group.

    python scripts/bench_threshold_checked.py [--out profiles/threshold_checked.json] [--reps 5] [--log2-groups 14,17]

Call time through Engine (host clock around the synchronous calls, the packing of the per-group byte strings and, for the
composition, the host's selection included).  The two routes are timed alternately, min of --reps repetitions after one warm-up
each, max - min recorded as the spread; kernel times from the engine's HIP-event profile in a run of their own.  Before any
timing the outputs of both routes are checked for equality (signatures, used shares), and the signatures verify under C_0."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
N_PER_GROUP, T = 7, 5


def b32(k):
    return int(k).to_bytes(32, "big")


def profile_of(eng, fn):
    eng.profile_reset(); eng.profile_enable(True)
    fn()
    eng.profile_enable(False)
    return {name: {"launches": v["launches"], "ms": round(v["total_ms"], 3)} for name, v in eng.profile_read().items()}


def make(eng, rnd, n_groups, bad_every, dst):
    coefs = b"".join(b32(rnd.randrange(1, R)) for _ in range(T * n_groups))
    cm = eng.sk_to_pk_batch(coefs, T * n_groups)
    commit_sets = [cm[128 * T * g:128 * T * (g + 1)] for g in range(n_groups)]
    coef_sets = [coefs[32 * T * g:32 * T * (g + 1)] for g in range(n_groups)]
    id_sets = [b"".join(map(b32, range(1, N_PER_GROUP + 1)))] * n_groups
    shares, st = eng.fr_poly_eval_batch(coef_sets, id_sets)
    assert st == bytes(n_groups)
    msgs = [b"checked %08d" % g for g in range(n_groups)]
    rep_msgs = [m for m in msgs for _ in range(N_PER_GROUP)]
    bad = []
    if bad_every:
        for g in range(bad_every - 1, n_groups, bad_every):
            i = N_PER_GROUP * g + (g // bad_every) % T
            rep_msgs[i] = b"another message"
            bad.append(i)
    sigs = eng.sign_batch(shares, rep_msgs, dst)
    sig_sets = [sigs[64 * N_PER_GROUP * g:64 * N_PER_GROUP * (g + 1)] for g in range(n_groups)]
    return commit_sets, id_sets, sig_sets, msgs, bad


def composition(eng, commit_sets, id_sets, sig_sets, msgs, dst):
    n_groups = len(id_sets)
    bm, st = eng.threshold_verify_shares_batch(commit_sets, id_sets, sig_sets, msgs, dst)
    live = np.unpackbits(np.frombuffer(bm, dtype=np.uint8), bitorder="little")[:N_PER_GROUP * n_groups].reshape(n_groups, N_PER_GROUP)
    # the first T live shares of every group; a group with fewer keeps none
    rank = np.cumsum(live, axis=1)
    pick = (live == 1) & (rank <= T) & (rank[:, -1:] >= T)
    ids = np.frombuffer(b"".join(id_sets), dtype=np.uint8).reshape(n_groups, N_PER_GROUP, 32)
    sg = np.frombuffer(b"".join(sig_sets), dtype=np.uint8).reshape(n_groups, N_PER_GROUP, 64)
    cnt = pick.sum(axis=1)
    ends = np.cumsum(cnt)
    ids_t, sigs_t = ids[pick].tobytes(), sg[pick].tobytes()
    id_t = [ids_t[32 * (e - c):32 * e] for c, e in zip(cnt.tolist(), ends.tolist())]
    sig_t = [sigs_t[64 * (e - c):64 * e] for c, e in zip(cnt.tolist(), ends.tolist())]
    out, cst = eng.threshold_combine_batch(id_t, sig_t)
    return out, np.packbits(pick.reshape(-1), bitorder="little").tobytes(), st, cst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log2-groups", default="14,17")
    a = ap.parse_args()
    assert a.reps >= 5, "at least 5 repetitions"
    import blsbn254_loader
    M = blsbn254_loader.load()
    eng = M.Engine(0)
    dst = M.DEFAULT_DST
    rnd = random.Random(2025)
    result = {"timing": "host clock around the synchronous Engine calls (packing of the per-group byte strings and, for the composition, the host's selection "
                        "included); the two routes alternate, min of reps after one warm-up each; spread = max - min of the reps; kernel times from the "
                        "HIP-event profile in a run of their own",
              "reps": a.reps, "shares_per_group": N_PER_GROUP, "threshold": T, "ids": "1..7"}
    rows = []
    for lg in [int(x) for x in a.log2_groups.split(",")]:
        n_groups = 1 << lg
        for bad_every in (0, 16):
            commit_sets, id_sets, sig_sets, msgs, bad = make(eng, rnd, n_groups, bad_every, dst)
            args = (commit_sets, id_sets, sig_sets, msgs, dst)
            row = {"log2_groups": lg, "groups": n_groups, "shares": n_groups * N_PER_GROUP, "bad_partials": len(bad),
                   "bad": "none" if not bad_every else "one bad candidate among the first t in every 16th group"}
            # -- both routes give the same signatures over the same shares, and the signatures verify under C_0
            s0 = eng.threshold_checked_stats()
            out, used, st = eng.threshold_combine_checked_batch(*args)
            s1 = eng.threshold_checked_stats()
            c_out, c_used, c_st, c_cst = composition(eng, *args)
            assert st == c_st == c_cst == bytes(n_groups)
            assert out == c_out and used == c_used, "the checked combine and the composition differ"
            c0 = b"".join(c[:128] for c in commit_sets)
            assert eng.verify_batch(c0, msgs, out, dst) == np.packbits(np.ones(n_groups, dtype=np.uint8), bitorder="little").tobytes()
            row["stats"] = {k: s1[k] - s0[k] for k in s0}
            assert row["stats"]["fallback_groups"] == len(bad) and row["stats"]["verified_shares"] == N_PER_GROUP * len(bad)
            # -- alternate the two so that drift of the machine hits both alike
            tn, tc = [], []
            for _ in range(a.reps + 1):
                t0 = time.perf_counter(); eng.threshold_combine_checked_batch(*args); tn.append(time.perf_counter() - t0)
                t0 = time.perf_counter(); composition(eng, *args); tc.append(time.perf_counter() - t0)
            tn, tc = tn[1:], tc[1:]
            row.update({"checked_ms": round(1e3 * min(tn), 3), "checked_spread_ms": round(1e3 * (max(tn) - min(tn)), 3),
                        "composition_ms": round(1e3 * min(tc), 3), "composition_spread_ms": round(1e3 * (max(tc) - min(tc)), 3)})
            row["ratio"] = round(row["composition_ms"] / row["checked_ms"], 2)
            row["checked_faster_beyond_spread"] = bool(row["composition_ms"] - row["checked_ms"] > row["checked_spread_ms"] + row["composition_spread_ms"])
            row["pairing_equations"] = {"checked": n_groups + N_PER_GROUP * len(bad), "composition": n_groups * N_PER_GROUP}
            ph = profile_of(eng, lambda: eng.threshold_combine_checked_batch(*args))
            row["checked_kernels_ms"] = ph
            row["checked_kernels_total_ms"] = round(sum(v["ms"] for v in ph.values()), 3)
            ph = profile_of(eng, lambda: composition(eng, *args))
            row["composition_kernels_total_ms"] = round(sum(v["ms"] for v in ph.values()), 3)
            print(json.dumps({k: v for k, v in row.items() if k != "checked_kernels_ms"}), flush=True)
            rows.append(row)
    result["rows"] = rows
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
