"""Pairing-product checks over groups by random linear combination (blsbn254_pairing_check_batch_rlc) against the exact call
(blsbn254_pairing_check_batch, unchanged by the RLC work: its time IS the parent commit's) on one GPU, both in the same run:
    python scripts/bench_pairing_check_rlc.py --out profiles/pairing_check_rlc.json
Shapes: kzg4, kzg10, kzg14, kzg18 (2^k two-pair equations over two distinct Q), bls16 (2^16 two-pair equations over -G2gen and a
pool of 1024 Q), groth14 (2^14 four-pair equations, one fresh Q per equation and three fixed), each three ways: all honest, one
false equation, one false in every 16.  Equations are closed forms, P = [a] G1gen and Q = [b] G2gen with sum a_j b_j = 0 mod r; a
false one has 1 added to its first a.  Call time through Engine (seed = None, the production setting), host clock around the
synchronous call, min of --reps repetitions after one warm-up, max - min recorded as the spread; the bitmap of both calls is
checked against the pattern before anything is timed.  Per-kernel times of the RLC call come from the engine's HIP-event profile of
one further call.  On the one-false rows the cap S_max of the default rule S = min(S_max, N / (2 u)) is tried at 16, 64 and 256
(blsbn254_set_pairing_check_rlc_segments with the S that cap gives); all three times are recorded.  merge_gap: the number of pairs
whose exact time equals a small exact call's fixed cost, from this run's kzg10 and kzg18 honest rows.
The weigh kernel's two forms: the library as built runs the mixed-addition chain; a library built with -DPCR_WEIGH_PLAIN (Makefile:
PCRLC_FLAGS) and named by BLSBN254_LIB runs agr_mul_glv32_x2 on z = 1; --weigh-only prints pcr_weigh's time per shape and nothing
else, so the two runs are compared line by line."""
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
POOL = 1024
S_MAX_TRIED = (16, 64, 256)
KERNELS = ("g2_prepare", "kd_insert", "pcr_pairs", "pcr_eq", "pcr_weigh", "pcr_items", "g1_seg_sum", "miller_wide_1p", "miller_tri_1p", "miller_hpk1p", "miller_hpk2p",
           "miller_wide_1", "miller_tri_1", "miller_1", "pair_ok", "fp12_seg_prod", "fe_easy", "fe_hard_wide", "fe_tri_hard", "fe_expx_h1", "fe_expx_h2", "fe_expx", "fe_h3")
SHAPES = {"kzg4": ("kzg", 4), "kzg10": ("kzg", 10), "kzg14": ("kzg", 14), "kzg18": ("kzg", 18), "bls16": ("bls", 16), "groth14": ("groth", 14)}


def b32(k):
    return int(k).to_bytes(32, "big")


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return round(1e3 * min(ts), 3), round(1e3 * (max(ts) - min(ts)), 3)


def scalars(kind, n_eq, rnd):
    """(pairs per equation, the distinct b's, per pair its a and the index of its b): every equation holds"""
    if kind == "kzg":
        bs = [rnd.randrange(1, R), rnd.randrange(1, R)]
        inv = pow(bs[1], -1, R)
        a, kk = [], []
        for _ in range(n_eq):
            a0 = rnd.randrange(1, R)
            a += [a0, -a0 * bs[0] * inv % R]; kk += [0, 1]
        return 2, bs, a, kk
    if kind == "bls":
        bs = [R - 1] + [rnd.randrange(1, R) for _ in range(POOL)]
        a, kk = [], []
        for g in range(n_eq):
            k = 1 + g % POOL
            a1 = rnd.randrange(1, R)
            a += [a1 * bs[k] % R, a1]; kk += [0, k]                     # e(sig, -G2gen) e(H, pk) = 1
        return 2, bs, a, kk
    bs = [rnd.randrange(1, R) for _ in range(3 + n_eq)]
    a, kk = [], []
    for g in range(n_eq):
        x = [rnd.randrange(1, R) for _ in range(3)]
        a += x + [-(x[0] * bs[0] + x[1] * bs[1] + x[2] * bs[2]) * pow(bs[3 + g], -1, R) % R]; kk += [0, 1, 2, 3 + g]
    return 4, bs, a, kk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="kzg4,kzg10,kzg14,kzg18,bls16,groth14")
    ap.add_argument("--weigh-only", action="store_true")
    a = ap.parse_args()
    assert a.reps >= 5, "at least 5 repetitions"
    import blsbn254_loader
    M = blsbn254_loader.load()
    from oracle import oracle as O
    O.build()
    eng = M.Engine(0)
    G1, G2 = O.g1_generator(), O.g2_generator()
    rows = []
    for name in a.shapes.split(","):
        kind, lg = SHAPES[name]
        n_eq = 1 << lg
        rnd = random.Random(lg * 131 + len(kind))
        k, bs, av, kk = scalars(kind, n_eq, rnd)
        N, u = n_eq * k, len(bs)
        qs = eng.g2_mul_batch(G2 * u, b"".join(map(b32, bs)), u)
        g2 = np.frombuffer(qs, dtype=np.uint8).reshape(u, 128)[np.asarray(kk)].tobytes()
        off = np.arange(0, N + 1, k, dtype=np.uint64)
        for mode, bad in (("honest", []), ("one_false", [n_eq // 2]), ("1_in_16", list(range(15, n_eq, 16)))):
            am = list(av)
            want = np.ones(n_eq, dtype=np.uint8)
            for g in bad:
                am[k * g] = (am[k * g] + 1) % R
                want[g] = 0
            want = np.packbits(want, bitorder="little").tobytes()
            g1 = eng.g1_mul_batch(G1 * N, b"".join(map(b32, am)), N)
            rlc = lambda: eng.pairing_check_batch_rlc(g1, g2, off)
            exact = lambda: eng.pairing_check_batch(g1, g2, off)
            eng.set_pairing_check_rlc_segments(0)
            s0 = eng.pairing_check_rlc_stats()
            assert rlc() == want, "the RLC bitmap differs from the pattern"
            s1 = eng.pairing_check_rlc_stats()
            row = {"shape": name, "equations": n_eq, "pairs_per_equation": k, "pairs": N, "distinct_q": u, "mode": mode, "false_equations": len(bad),
                   "stats_of_one_call": {x: s1[x] - s0[x] for x in s1}}
            eng.profile_reset(); eng.profile_enable(True)
            rlc()
            eng.profile_enable(False)
            prof = eng.profile_read()
            eng.profile_reset()
            row.update({"rlc_kernels_ms": {x: {"launches": prof[x]["launches"], "ms": round(prof[x]["total_ms"], 3)} for x in KERNELS if x in prof},
                        "rlc_kernel_total_ms": round(sum(v["total_ms"] for v in prof.values()), 3)})
            if a.weigh_only:
                print(json.dumps({"shape": name, "mode": mode, "lib": os.environ.get("BLSBN254_LIB", "as built"), "pcr_weigh_ms": row["rlc_kernels_ms"].get("pcr_weigh")}), flush=True)
                if mode == "honest":
                    rows.append(row)
                continue
            assert exact() == want, "the exact bitmap differs from the pattern"
            te, se = timed(exact, a.reps)
            tr, sr = timed(rlc, a.reps)
            row.update({"exact_ms": te, "exact_spread_ms": se, "rlc_ms": tr, "rlc_spread_ms": sr, "rlc_over_exact": round(tr / te, 3),
                        "rlc_below_exact_beyond_spreads": bool(te - tr > se + sr)})
            if mode == "one_false":
                tried = {}
                for s_max in S_MAX_TRIED:
                    S = min(s_max, N // (2 * u), n_eq)
                    eng.set_pairing_check_rlc_segments(S if S >= 2 else 1)
                    assert rlc() == want
                    t, sp = timed(rlc, a.reps)
                    tried[str(s_max)] = {"segments": S, "rlc_ms": t, "rlc_spread_ms": sp}
                eng.set_pairing_check_rlc_segments(0)
                row["s_max_tried"] = tried
            print(json.dumps(row), flush=True)
            rows.append(row)
    stats = eng.pairing_check_rlc_stats()
    eng.close()
    out = {"timing": "host clock around the synchronous call through Engine, min of reps after one warm-up; spread = max - min of the reps; "
                     "both calls in the same run, the exact call first",
           "exact": "blsbn254_pairing_check_batch, unchanged by the RLC call: the parent commit's number",
           "reps": a.reps, "pool": POOL, "s_max_tried": list(S_MAX_TRIED), "rows": rows, "stats": stats}
    by = {(r["shape"], r["mode"]): r for r in rows if "exact_ms" in r}
    if ("kzg10", "honest") in by and ("kzg18", "honest") in by:
        small, large = by[("kzg10", "honest")], by[("kzg18", "honest")]
        per_pair = large["exact_ms"] / large["pairs"]
        out["merge_gap"] = {"small_exact_call_ms": small["exact_ms"], "exact_ms_per_pair_at_2^18x2": round(per_pair, 7),
                            "pairs_whose_exact_time_is_a_small_call": int(small["exact_ms"] / per_pair)}
        print(json.dumps({"merge_gap": out["merge_gap"]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
