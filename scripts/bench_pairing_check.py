"""Pairing-product equations over groups of pairs (blsbn254_pairing_check_batch) on one GPU: equations per second (host clock
around the synchronous call, after a warm-up), per-phase kernel ms from profile_read, the same inputs through the host
composition g2_check_batch + miller_loop_batch + gt_mul_batch folds + final_exponentiation + a compare on the host (with the
speedup), and per-pair pairing_batch time for scale.  Equations P_j = [a_j] G1, Q_j = [b_j] G2 with sum_j a_j b_j = 0 mod r,
every 16th broken by one scalar; both paths must give the expected bitmap.
    python scripts/bench_pairing_check.py [--out profiles/pairing_check.json] [--reps 3]"""
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
ONE = (1).to_bytes(32, "big") + bytes(352)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return 1e3 * min(ts)


def equations(eng, O, rnd, n_eq, k):
    """n_eq equations of k pairs (equation-major), expected bits"""
    a, b, holds = [], [], []
    for g in range(n_eq):
        ag = [rnd.randrange(1, R) for _ in range(k)]
        bg = [rnd.randrange(1, R) for _ in range(k - 1)]
        rest = sum(x * y for x, y in zip(ag, bg)) % R
        ok = g % 16 != 15
        bg.append((-rest + (0 if ok else 1)) * pow(ag[-1], -1, R) % R)
        a += ag; b += bg; holds.append(ok)
    n = n_eq * k
    P = eng.g1_mul_batch(O.g1_generator() * n, b"".join(x.to_bytes(32, "big") for x in a), n)
    Q = eng.g2_mul_batch(O.g2_generator() * n, b"".join(x.to_bytes(32, "big") for x in b), n)
    bm = np.packbits(np.array(holds, dtype=np.uint8), bitorder="little").tobytes()
    return P, Q, bm


def composition(eng, P, Q, n_eq, k):
    """the same check through the existing entry points, with the segmenting done on the host"""
    n = n_eq * k
    sub = np.unpackbits(np.frombuffer(eng.g2_check_batch(Q, n), dtype=np.uint8), bitorder="little")[:n].reshape(n_eq, k).all(axis=1)
    ml = np.frombuffer(eng.miller_loop_batch(P, Q, n), dtype=np.uint8).reshape(n_eq, k, 384)
    acc = ml[:, 0].tobytes()
    for j in range(1, k):
        acc = eng.gt_mul_batch(acc, ml[:, j].tobytes(), n_eq)
    gt = np.frombuffer(eng.final_exponentiation(acc, n_eq), dtype=np.uint8).reshape(n_eq, 384)
    one = (gt == np.frombuffer(ONE, dtype=np.uint8)).all(axis=1)
    return np.packbits((one & sub).astype(np.uint8), bitorder="little").tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="10x2,14x2,18x2,16x4", help="log2(equations) x pairs per equation")
    a = ap.parse_args()
    import blsbn254_loader
    M = blsbn254_loader.load()
    from oracle import oracle as O
    O.build()
    eng = M.Engine(0)
    rnd = random.Random(1)
    rows = []
    for shape in a.shapes.split(","):
        lg, k = (int(x) for x in shape.split("x"))
        n_eq = 1 << lg
        n = n_eq * k
        P, Q, want = equations(eng, O, rnd, n_eq, k)
        off = np.arange(0, n + 1, k, dtype=np.uint64)
        got = eng.pairing_check_batch(P, Q, off)
        comp = composition(eng, P, Q, n_eq, k)
        assert got == want and comp == want, "bitmap differs from the closed form"
        t_fused = timed(lambda: eng.pairing_check_batch(P, Q, off), a.reps)
        eng.profile_reset(); eng.profile_enable(True)
        eng.pairing_check_batch(P, Q, off)
        eng.profile_enable(False)
        phases = {name: {"launches": v["launches"], "ms": round(v["total_ms"], 3)} for name, v in eng.profile_read().items()}
        t_comp = timed(lambda: composition(eng, P, Q, n_eq, k), a.reps)
        t_pair = timed(lambda: eng.pairing_batch(P, Q, n), 1)
        row = {"log2_equations": lg, "equations": n_eq, "pairs_per_equation": k, "pairs": n,
               "fused_ms": round(t_fused, 3), "equations_per_s": round(n_eq / (t_fused / 1e3)),
               "kernel_phases_ms": phases, "kernel_total_ms": round(sum(v["ms"] for v in phases.values()), 3),
               "composition_ms": round(t_comp, 3), "fused_over_composition": round(t_fused / t_comp, 3),
               "speedup": round(t_comp / t_fused, 2),
               "pairing_batch_ms": round(t_pair, 3), "pairing_batch_us_per_pair": round(1e3 * t_pair / n, 4)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    eng.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"composition": "g2_check_batch + miller_loop_batch + (k - 1) gt_mul_batch folds + final_exponentiation + compare on the host",
                       "timing": "host clock around the synchronous call, min of reps after one warm-up", "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
