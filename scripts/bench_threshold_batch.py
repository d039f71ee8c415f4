"""Threshold combine over groups of partial signatures (blsbn254_threshold_combine_batch) on one GPU.  Per shape (groups x shares):
the batched call (host clock around the synchronous call, min of reps after a warm-up; groups/s, shares/s), per-phase kernel ms
from profile_read, the loop of blsbn254_threshold_combine over the same groups on the same context (for more than 2^12 groups
the loop runs on the first 2^12 and the figure is per group x groups, marked extrapolated), and g1_mul_batch over the same N
points for scale (with its k_g1_mul kernel time).  The two sides of the comparison alternate inside the process.  Results are
checked before anything is timed: shares [f_g(x_i)] H(m_g) of a polynomial of degree <= 6, expected [f_g(0)] H(m_g).

--sweep-lib <a build with the hand-over lifted> adds the sweep that places the hand-over size: 16 equal groups per call at
t = 64 .. 4096, the lane-per-share kernels (that build) against the loop of single calls.  The build is
    make -C bls-bn254_amd VARIANT=_nohandover THBATCH_HOST_FLAGS=-DBN_TH_BATCH_TBIG=8388608
    python scripts/bench_threshold_batch.py [--out profiles/threshold_batch.json] [--reps 3] [--sweep-lib bls-bn254_amd/libblsbn254_hip_nohandover.so]"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
LOOP_MAX = 1 << 12


def b32(k):
    return int(k).to_bytes(32, "big")


def alternating(fa, fb, reps):
    """min over reps of each side, a b a b ..., after one warm-up of each"""
    fa(); fb()
    ta, tb = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); fa(); ta.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); fb(); tb.append(time.perf_counter() - t0)
    return 1e3 * min(ta), 1e3 * min(tb)


def groups(eng, rnd, sizes, dst):
    """(id_sets, sig_sets, expected signatures): f_g of degree min(t, 7) - 1, ids drawn from 1 .. t + 3"""
    id_sets, sks, share_msgs, secrets, msgs = [], [], [], [], []
    for g, t in enumerate(sizes):
        c = [rnd.randrange(1, R) for _ in range(min(t, 7))]
        ids = rnd.sample(range(1, t + 4), t)
        m = b"bench %d" % g
        id_sets.append(b"".join(map(b32, ids)))
        for x in ids:
            acc = 0
            for k in reversed(c):
                acc = (acc * x + k) % R
            sks.append(acc)
        share_msgs += [m] * t
        secrets.append(c[0]); msgs.append(m)
    sigs = eng.sign_batch(b"".join(map(b32, sks)), share_msgs, dst)
    sig_sets, pos = [], 0
    for t in sizes:
        sig_sets.append(sigs[64 * pos:64 * (pos + t)])
        pos += t
    return id_sets, sig_sets, eng.sign_batch(b"".join(map(b32, secrets)), msgs, dst)


def phases_of(eng, fn):
    eng.profile_reset(); eng.profile_enable(True)
    fn()
    eng.profile_enable(False)
    return {name: {"launches": v["launches"], "ms": round(v["total_ms"], 3)} for name, v in eng.profile_read().items()}


def loop_single(eng, id_sets, sig_sets, m):
    return b"".join(eng.threshold_combine(id_sets[g], sig_sets[g], len(id_sets[g]) // 32) for g in range(m))


def engine_of(M, path):
    """an Engine on another build of the library (BLSBN254_LIB is read when the library is first loaded: load it aside)"""
    mod = sys.modules[M.Engine.__module__]
    saved, mod._lib = mod._lib, None
    os.environ["BLSBN254_LIB"] = path
    try:
        return M.Engine(0)
    finally:
        mod._lib = saved
        del os.environ["BLSBN254_LIB"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="10x7,14x7,17x7,12x67,8x667,4x2000,ragged,3x5000",
                    help="log2(groups) x shares per group; ragged = 4096 groups of 3 .. 100; 3x5000 lies beyond the hand-over size (single-group pipeline)")
    ap.add_argument("--sweep-lib", default=None)
    ap.add_argument("--sweep", default="64,128,256,512,1024,2048,4096")
    a = ap.parse_args()
    import blsbn254_loader
    M = blsbn254_loader.load()
    dst = M.DEFAULT_DST
    eng = M.Engine(0)
    t_big = eng.threshold_batch_stats()["t_big"]
    rows, sweep = [], []
    for shape in [s for s in a.shapes.split(",") if s]:
        rnd = random.Random(1)
        if shape == "ragged":
            sizes = [rnd.randint(3, 100) for _ in range(4096)]
        else:
            lg, t = (int(x) for x in shape.split("x"))
            sizes = [t] * (1 << lg)
        ng, n = len(sizes), sum(sizes)
        id_sets, sig_sets, want = groups(eng, rnd, sizes, dst)
        s0 = eng.threshold_batch_stats()
        out, st = eng.threshold_combine_batch(id_sets, sig_sets)
        s1 = eng.threshold_batch_stats()
        assert st == bytes(ng) and out == want, "the batched call differs from the closed form"
        m = min(ng, LOOP_MAX)
        assert loop_single(eng, id_sets, sig_sets, m) == want[:64 * m], "the loop of single calls differs from the closed form"
        t_batch, t_loop = alternating(lambda: eng.threshold_combine_batch(id_sets, sig_sets), lambda: loop_single(eng, id_sets, sig_sets, m), a.reps)
        ph = phases_of(eng, lambda: eng.threshold_combine_batch(id_sets, sig_sets))
        pts = b"".join(sig_sets); ks = b"".join(b32(rnd.randrange(R)) for _ in range(n))
        eng.g1_mul_batch(pts, ks, n)
        t0 = time.perf_counter(); eng.g1_mul_batch(pts, ks, n); t_mul = 1e3 * (time.perf_counter() - t0)
        ph_mul = phases_of(eng, lambda: eng.g1_mul_batch(pts, ks, n))
        loop_ms = t_loop * ng / m
        row = {"shape": shape, "groups": ng, "shares": n, "batched_groups": s1["batched_groups"] - s0["batched_groups"],
               "single_groups": s1["single_groups"] - s0["single_groups"], "launches": s1["launches"] - s0["launches"],
               "batched_ms": round(t_batch, 3), "groups_per_s": round(ng / (t_batch / 1e3)), "shares_per_s": round(n / (t_batch / 1e3)),
               "kernel_phases_ms": ph, "kernel_total_ms": round(sum(v["ms"] for v in ph.values()), 3),
               "loop_of_single_calls_ms": round(loop_ms, 3), "loop_groups_timed": m, "loop_extrapolated": m != ng,
               "loop_us_per_group": round(1e3 * t_loop / m, 2), "batched_over_loop": round(t_batch / loop_ms, 4), "speedup": round(loop_ms / t_batch, 2),
               "g1_mul_batch_ms": round(t_mul, 3), "g1_mul_kernel_ms": ph_mul.get("g1_mul", {}).get("ms"),
               "g1_smul_glv_kernel_ms": ph.get("g1_smul_glv", {}).get("ms")}
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.sweep_lib:
        e2 = engine_of(M, os.path.abspath(a.sweep_lib))
        ts = [int(x) for x in a.sweep.split(",")]
        assert e2.threshold_batch_stats()["t_big"] >= max(ts), "the sweep needs a build with the hand-over beyond its largest group"
        for t in ts:
            rnd = random.Random(t)
            sizes = [t] * 16
            id_sets, sig_sets, want = groups(eng, rnd, sizes, dst)
            s0 = e2.threshold_batch_stats()
            out, st = e2.threshold_combine_batch(id_sets, sig_sets)
            assert e2.threshold_batch_stats()["batched_groups"] - s0["batched_groups"] == 16
            assert st == bytes(16) and out == want and loop_single(eng, id_sets, sig_sets, 16) == want
            t_batch, t_loop = alternating(lambda: e2.threshold_combine_batch(id_sets, sig_sets), lambda: loop_single(eng, id_sets, sig_sets, 16), a.reps)
            ph = phases_of(e2, lambda: e2.threshold_combine_batch(id_sets, sig_sets))
            row = {"t": t, "groups": 16, "lane_per_share_ms": round(t_batch, 3), "loop_of_single_calls_ms": round(t_loop, 3),
                   "loop_wins": t_loop < t_batch, "kernel_phases_ms": {k: v["ms"] for k, v in ph.items()}}
            print(json.dumps(row), flush=True)
            sweep.append(row)
        e2.close()
    eng.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"timing": "host clock around the synchronous call, min of reps after one warm-up, the two sides alternating",
                       "loop": "blsbn254_threshold_combine per group on the same context; beyond 4096 groups timed on the first 4096 and scaled",
                       "t_big": t_big, "rows": rows, "hand_over_sweep": sweep}, f, indent=1)


if __name__ == "__main__":
    main()
