"""Public key shares from Feldman commitments (blsbn254_g2_poly_eval_batch) and the check of partial signatures against them
(blsbn254_threshold_verify_shares_batch) on one GPU, next to their yardsticks in the same build: g2_mul_batch on the same number
of points (one windowed multiplication = 332 group operations, against 2 x bits x (t - 1) of the Horner evaluation) and
verify_batch on precomputed key shares with the group's message replicated per share (the difference is what the evaluation
costs inside the call).

The only way to get these points from the parent commit is one g2_msm call of t terms per share with host-computed powers of
the id; that uses entry points the parent has and is to be measured on the PARENT commit's build over 2^10 shares:
    BLSBN254_LIB=<parent build>.so python scripts/bench_threshold_deal.py --phase parent --out parent.json
    python scripts/bench_threshold_deal.py --phase deal --parent parent.json --out profiles/threshold_deal.json
Call time through Engine (host clock around the synchronous call, the packing of the per-group byte strings included, min of
--reps repetitions after one warm-up, max - min recorded as the spread); kernel times from the engine's HIP-event profile in a
run of their own.  Every path's output is checked before it is timed: the key shares against sk_to_pk_batch of the shares
fr_poly_eval_batch gives (and a few of those against Python integers), the bitmaps against the pattern of corrupted shares."""
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


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return 1e3 * min(ts), 1e3 * (max(ts) - min(ts))


def poly_eval(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def profile_of(eng, fn):
    eng.profile_reset(); eng.profile_enable(True)
    fn()
    eng.profile_enable(False)
    return {name: {"launches": v["launches"], "ms": round(v["total_ms"], 3)} for name, v in eng.profile_read().items()}


def make_groups(eng, rnd, n_groups, kind):
    """n_groups groups of N_PER_GROUP ids (1 .. 7, or random in [1, r)) over polynomials of T coefficients: commitment sets, id
    sets, the coefficients and ids as integers"""
    coefs = [[rnd.randrange(1, R) for _ in range(T)] for _ in range(n_groups)]
    flat = b"".join(b32(c) for cs in coefs for c in cs)
    cm = eng.sk_to_pk_batch(flat, T * n_groups)
    commit_sets = [cm[128 * T * g:128 * T * (g + 1)] for g in range(n_groups)]
    if kind == "small":
        ids = [list(range(1, N_PER_GROUP + 1))] * n_groups
    else:
        ids = [[rnd.randrange(1, R) for _ in range(N_PER_GROUP)] for _ in range(n_groups)]
    id_sets = [b"".join(map(b32, x)) for x in ids]
    return coefs, ids, commit_sets, id_sets, [flat[32 * T * g:32 * T * (g + 1)] for g in range(n_groups)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", choices=["parent", "deal"], required=True)
    ap.add_argument("--parent", default=None, help="the JSON written by --phase parent (merged by --phase deal)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log2-groups", default="14,17")
    a = ap.parse_args()
    assert a.reps >= 5, "at least 5 repetitions"
    import blsbn254_loader
    M = blsbn254_loader.load()
    eng = M.Engine(0)
    dst = M.DEFAULT_DST
    rnd = random.Random(2024)
    result = {"timing": "host clock around the synchronous Engine call (packing of the per-group byte strings included), min of reps after one "
                        "warm-up; spread = max - min of the reps; kernel times from the HIP-event profile in a run of their own",
              "reps": a.reps, "phase": a.phase, "shares_per_group": N_PER_GROUP, "coefficients_per_group": T}
    if a.phase == "parent":
        # one g2_msm of T terms per share, powers of the id computed on the host: 2^10 shares (147 groups of 7, cut at 1024)
        n_groups = 147
        coefs, ids, commit_sets, _, _ = make_groups(eng, rnd, n_groups, "small")
        shares = [(g, i) for g in range(n_groups) for i in range(N_PER_GROUP)][:1 << 10]
        powers = [b"".join(b32(pow(ids[g][i], j, R)) for j in range(T)) for g, i in shares]

        def loop():
            return [eng.g2_msm(commit_sets[g], powers[k], T) for k, (g, _) in enumerate(shares)]
        got = loop()
        want = eng.sk_to_pk_batch(b"".join(b32(poly_eval(coefs[g], ids[g][i])) for g, i in shares), len(shares))
        assert b"".join(got) == want, "the msm loop's key shares differ from sk_to_pk of the shares"
        t, sp = timed(loop, a.reps)
        result["msm_loop"] = {"shares": len(shares), "ms": round(t, 3), "spread_ms": round(sp, 3), "us_per_share": round(1e3 * t / len(shares), 2)}
        print(json.dumps(result["msm_loop"]), flush=True)
    else:
        rows = []
        for lg in [int(x) for x in a.log2_groups.split(",")]:
            n_groups = 1 << lg
            n = n_groups * N_PER_GROUP
            for kind in ("small", "full"):
                coefs, ids, commit_sets, id_sets, coef_sets = make_groups(eng, rnd, n_groups, kind)
                row = {"log2_groups": lg, "groups": n_groups, "shares": n, "ids": "1..7" if kind == "small" else "random in [1, r)"}
                # -- correctness of every path before its timing
                shares, st = eng.fr_poly_eval_batch(coef_sets, id_sets)
                assert st == bytes(n_groups)
                for g in rnd.sample(range(n_groups), 8):
                    assert shares[32 * N_PER_GROUP * g:32 * N_PER_GROUP * (g + 1)] == b"".join(b32(poly_eval(coefs[g], x)) for x in ids[g])
                want_pks = eng.sk_to_pk_batch(shares, n)
                pks, st = eng.g2_poly_eval_batch(commit_sets, id_sets)
                assert st == bytes(n_groups) and pks == want_pks, "key shares differ from sk_to_pk of the shares"
                row["id_bits"] = eng.threshold_deal_stats()["id_bits"]
                row["group_ops_per_share"] = 2 * row["id_bits"] * (T - 1) + (T - 1)
                t, sp = timed(lambda: eng.g2_poly_eval_batch(commit_sets, id_sets), a.reps)
                row.update({"g2_poly_eval_ms": round(t, 3), "g2_poly_eval_spread_ms": round(sp, 3)})
                t0 = time.perf_counter(); b"".join(commit_sets); b"".join(id_sets); eng._group_offsets(commit_sets, 128, ""); eng._group_offsets(id_sets, 32, "")
                row["host_packing_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
                ph = profile_of(eng, lambda: eng.g2_poly_eval_batch(commit_sets, id_sets))
                row["g2_poly_eval_kernels_ms"] = ph
                row["k_g2_poly_eval_ms"] = ph["g2_poly_eval"]["ms"]
                # -- the yardstick: one windowed multiplication per point, same number of points, same build
                pts = (b"".join(commit_sets) * 2)[:128 * n]
                prods = b"".join(b32(int.from_bytes(shares[32 * i:32 * i + 32], "big") * coefs[i // T][i % T] % R) for i in range(64))
                assert eng.g2_mul_batch(pts[:128 * 64], shares[:32 * 64], 64) == eng.sk_to_pk_batch(prods, 64)      # [s] [a] G2 = [s a] G2
                t, sp = timed(lambda: eng.g2_mul_batch(pts, shares, n), a.reps)
                row.update({"g2_mul_batch_ms": round(t, 3), "g2_mul_batch_spread_ms": round(sp, 3), "g2_mul_group_ops_per_point": 332})
                row["k_g2_mul_ms"] = profile_of(eng, lambda: eng.g2_mul_batch(pts, shares, n))["g2_mul"]["ms"]
                row["poly_eval_below_g2_mul_beyond_spread"] = bool(row["g2_mul_batch_ms"] - row["g2_poly_eval_ms"] > row["g2_mul_batch_spread_ms"] + row["g2_poly_eval_spread_ms"])
                # -- the check of partial signatures: every 16th group holds one share signed with a neighbour's key
                sk = bytearray(shares)
                expect = np.ones(n, dtype=np.uint8)
                for g in range(15, n_groups, 16):
                    i = N_PER_GROUP * g + (g // 16) % N_PER_GROUP
                    j = i + 1 if i % N_PER_GROUP < N_PER_GROUP - 1 else i - 1
                    sk[32 * i:32 * i + 32] = shares[32 * j:32 * j + 32]
                    expect[i] = 0
                want_bm = np.packbits(expect, bitorder="little").tobytes()
                msgs = [b"deal %08d" % g for g in range(n_groups)]
                rep_msgs = [m for m in msgs for _ in range(N_PER_GROUP)]
                sigs = eng.sign_batch(bytes(sk), rep_msgs, dst)
                sig_sets = [sigs[64 * N_PER_GROUP * g:64 * N_PER_GROUP * (g + 1)] for g in range(n_groups)]
                bm, st = eng.threshold_verify_shares_batch(commit_sets, id_sets, sig_sets, msgs, dst)
                assert st == bytes(n_groups) and bm == want_bm, "the bitmap differs from the pattern of corrupted shares"
                assert eng.verify_batch(pks, rep_msgs, sigs, dst) == want_bm
                # alternate the two so that drift of the machine hits both alike
                tv, tb = [], []
                for _ in range(a.reps + 1):
                    t0 = time.perf_counter(); eng.threshold_verify_shares_batch(commit_sets, id_sets, sig_sets, msgs, dst); tv.append(time.perf_counter() - t0)
                    t0 = time.perf_counter(); eng.verify_batch(pks, rep_msgs, sigs, dst); tb.append(time.perf_counter() - t0)
                tv, tb = tv[1:], tb[1:]
                row.update({"verify_shares_ms": round(1e3 * min(tv), 3), "verify_shares_spread_ms": round(1e3 * (max(tv) - min(tv)), 3),
                            "verify_batch_ms": round(1e3 * min(tb), 3), "verify_batch_spread_ms": round(1e3 * (max(tb) - min(tb)), 3)})
                row["evaluation_inside_the_call_ms"] = round(row["verify_shares_ms"] - row["verify_batch_ms"], 3)
                print(json.dumps(row), flush=True)
                rows.append(row)
        result["rows"] = rows
        if a.parent:
            result["parent_msm_loop"] = json.load(open(a.parent))["msm_loop"]
        result["stats"] = eng.threshold_deal_stats()
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
