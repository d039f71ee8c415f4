"""Multi-scalar multiplication sum_i [k_i] P_i (blsbn254_g1_msm / blsbn254_g2_msm) on one GPU: call time (host clock around the
synchronous call, after a warm-up), per-phase kernel ms from profile_read, the chosen window c, the element-wise baseline
(g1_mul_batch + aggregate_sigs / g2_mul_batch + aggregate_pks) on the same inputs, the every-scalar-equal case, and the achieved
rate of bucket additions and of field-multiply MADs against the measured v_mad peak.
    python scripts/bench_msm.py [--out profiles/msm.json] [--reps 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
MAD_PER_FPMUL = 162                     # fp29.h: 81 operand + 81 reduction v_mad_i64_i32 per Fp multiply
FPMUL = {"g1": {"madd": 11, "add": 12, "dbl": 6}, "g2": {"madd": 11 * 3, "add": 12 * 3, "dbl": 6 * 3}}   # Fp2 mul = 3 Fp muls


def scalars(rng, n):
    b = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    b[:, 0] &= 0x2f                                            # < 0x30 00.. < r
    return b.tobytes()


def window(n, halves, bits):
    best, cost = 2, None
    for c in range(2, 17):
        w = (bits + c) // c
        v = w * (halves * n + 1.5 * (1 << c))
        if cost is None or v < cost:
            best, cost = c, v
    return best


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return 1e3 * min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--g1", default="10,14,18,20,22")
    ap.add_argument("--g2", default="10,14,18")
    a = ap.parse_args()
    import blsbn254_loader
    M = blsbn254_loader.load()
    eng = M.Engine(0)
    peak = eng.valu_peak()
    rng = np.random.default_rng(1)
    rows = []
    for grp, logs in (("g1", a.g1), ("g2", a.g2)):
        g2 = grp == "g2"
        sz, halves, bits = (128, 1, 254) if g2 else (64, 2, 128)
        from oracle import oracle as O
        O.build()
        gen = O.g2_generator() if g2 else O.g1_generator()
        mul_batch = eng.g2_mul_batch if g2 else eng.g1_mul_batch
        msm = eng.g2_msm if g2 else eng.g1_msm
        agg = eng.aggregate_pks if g2 else eng.aggregate_sigs
        for lg in [int(x) for x in logs.split(",") if x]:
            n = 1 << lg
            pts = mul_batch(gen * n, scalars(rng, n), n)
            ks = scalars(rng, n)
            c = window(n, halves, bits)
            t_msm = timed(lambda: msm(pts, ks, n), a.reps)
            eng.profile_reset(); eng.profile_enable(True)
            msm(pts, ks, n)
            eng.profile_enable(False)
            phases = {k: round(v["total_ms"], 4) for k, v in eng.profile_read().items()}
            base = None
            if lg <= 20:
                base = timed(lambda: agg(mul_batch(pts, ks, n), n), 1)
            st0 = eng.msm_stats(); msm(pts, ks, n); st1 = eng.msm_stats()
            entries = st1["entries"] - st0["entries"]
            w = (bits + c) // c
            b = 1 << (c - 1)
            ops = FPMUL[grp]
            fpm = entries * ops["madd"] + (entries / 32 + w * b) * ops["add"] + w * b * 2 * ops["add"] + bits * ops["dbl"]
            row = {"group": grp, "log2_n": lg, "n": n, "c": c, "msm_ms": round(t_msm, 3), "phases_ms": phases,
                   "bucket_entries": entries, "madd_per_s": entries / (t_msm / 1e3), "fp_muls": fpm,
                   "mad_per_s": fpm * MAD_PER_FPMUL / (t_msm / 1e3), "mad_peak_per_s": peak}
            if base is not None:
                row["mul_batch_plus_sum_ms"] = round(base, 3)
                row["speedup"] = round(base / t_msm, 2)
            if lg == 20 and not g2:
                keq = scalars(rng, 1) * n
                row["equal_scalars_ms"] = round(timed(lambda: msm(pts, keq, n), a.reps), 3)
                eng.profile_reset(); eng.profile_enable(True); msm(pts, keq, n); eng.profile_enable(False)
                row["equal_scalars_phases_ms"] = {k: round(v["total_ms"], 4) for k, v in eng.profile_read().items()}
            print(json.dumps(row), flush=True)
            rows.append(row)
    eng.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"window_rule": "c = argmin_c ceil((bits + 1) / c) (halves n + 1.5 2^c), bits = 128 (G1, GLV) / 254 (G2)",
                       "small_n_path": "none: the bucket path serves every n", "chunk_L": 32, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
