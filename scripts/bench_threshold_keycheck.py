"""Dealt key shares checked against Feldman commitments (blsbn254_threshold_verify_key_shares_batch) on one GPU, next to the
composition the parent commit offers for the same bits, in the same build and on the same inputs through Engine:
sk_to_pk_batch(shares) + g2_poly_eval_batch + a byte compare of 2 x 128 B per share on the host.

Protocol: per row 3 warm-ups and 20 timed repetitions of each form, ALTERNATING; median and interquartile spread
of the wall time (host clock around synchronous Engine calls, the packing of the per-group byte strings included).  Kernel times
come from the context's HIP-event profile in a pass of their own.  Every form's bitmap is checked against the Python pattern of
corrupted shares before it is timed.  Condition on the two short-id rows of 2^14 and 2^17 groups: the new call's median lies
below the composition's by more than the two spreads together.

    python scripts/bench_threshold_keycheck.py --out profiles/threshold_keycheck.json
    BLSBN254_LIB=<a build with -DBN_KC_WINDOW_BITS=4>.so python scripts/bench_threshold_keycheck.py --only-new --out w4.json
    python scripts/bench_threshold_keycheck.py --merge-window w4.json --out profiles/threshold_keycheck.json   (after the first)"""
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
WARMUP, REPS = 3, 20


def b32(k):
    return int(k).to_bytes(32, "big")


def poly_eval(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def stats(ts):
    a = np.sort(1e3 * np.asarray(ts))
    q1, med, q3 = (float(np.percentile(a, p)) for p in (25, 50, 75))
    return {"median_ms": round(med, 3), "spread_ms": round(q3 - q1, 3), "q1_ms": round(q1, 3), "q3_ms": round(q3, 3), "min_ms": round(float(a[0]), 3),
            "max_ms": round(float(a[-1]), 3)}


def profile_of(eng, fn):
    eng.profile_reset(); eng.profile_enable(True)
    fn()
    eng.profile_enable(False)
    return {name: {"launches": v["launches"], "ms": round(v["total_ms"], 3)} for name, v in eng.profile_read().items()}


def make_row(eng, rnd, n_groups, kind, wrong_every):
    """n_groups x (7 ids, 5 coefficients): the commitment, id and share sets and the Python pattern of the bits"""
    coefs = [[rnd.randrange(1, R) for _ in range(T)] for _ in range(n_groups)]
    flat = b"".join(b32(c) for cs in coefs for c in cs)
    cm = eng.sk_to_pk_batch(flat, T * n_groups)
    commit_sets = [cm[128 * T * g:128 * T * (g + 1)] for g in range(n_groups)]
    if kind == "small":
        ids = [list(range(1, N_PER_GROUP + 1))] * n_groups
    else:
        ids = [[rnd.randrange(1, R) for _ in range(N_PER_GROUP)] for _ in range(n_groups)]
    id_sets = [b"".join(map(b32, x)) for x in ids]
    coef_sets = [flat[32 * T * g:32 * T * (g + 1)] for g in range(n_groups)]
    shares, st = eng.fr_poly_eval_batch(coef_sets, id_sets)
    assert st == bytes(n_groups)
    for g in rnd.sample(range(n_groups), min(8, n_groups)):          # the dealer's kernel against Python integers
        assert shares[32 * N_PER_GROUP * g:32 * N_PER_GROUP * (g + 1)] == b"".join(b32(poly_eval(coefs[g], x)) for x in ids[g])
    shares = bytearray(shares)
    expect = np.ones(n_groups * N_PER_GROUP, dtype=np.uint8)
    if wrong_every:
        for g in range(wrong_every - 1, n_groups, wrong_every):
            i = N_PER_GROUP * g + (g // wrong_every) % N_PER_GROUP
            shares[32 * i:32 * i + 32] = b32((int.from_bytes(shares[32 * i:32 * i + 32], "big") + 1) % R)
            expect[i] = 0
    share_sets = [bytes(shares[32 * N_PER_GROUP * g:32 * N_PER_GROUP * (g + 1)]) for g in range(n_groups)]
    return commit_sets, id_sets, share_sets, np.packbits(expect, bitorder="little").tobytes()


def composition(eng, commit_sets, id_sets, share_sets):
    flat = b"".join(share_sets)
    n = len(flat) // 32
    lhs = np.frombuffer(eng.sk_to_pk_batch(flat, n), dtype=np.uint8).reshape(n, 128)
    rhs, st = eng.g2_poly_eval_batch(commit_sets, id_sets)
    eq = (lhs == np.frombuffer(rhs, dtype=np.uint8).reshape(n, 128)).all(axis=1)
    return np.packbits(eq, bitorder="little").tobytes(), st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-new", action="store_true", help="time the new call alone (a build with another window width)")
    ap.add_argument("--merge-window", default=None, help="a JSON written with --only-new on another build: merged into --out, nothing is run")
    ap.add_argument("--rows", default="14:small:0,17:small:0,14:small:16,17:small:16,14:full:0,4:small:0")
    a = ap.parse_args()
    if a.merge_window:
        out = json.load(open(a.out)); other = json.load(open(a.merge_window))
        out["other_window"] = {"window_bits": other["window_bits"], "table_bytes": other["table_bytes"],
                               "rows": [{k: r[k] for k in ("log2_groups", "ids", "wrong_every", "new_call", "k_td_key_check_ms") if k in r} for r in other["rows"]]}
        for r, o in zip(out["rows"], other["rows"]):
            assert (r["log2_groups"], r["ids"], r["wrong_every"]) == (o["log2_groups"], o["ids"], o["wrong_every"])
            r["k_td_key_check_other_window_over_this"] = round(o["k_td_key_check_ms"] / r["k_td_key_check_ms"], 3)
        json.dump(out, open(a.out, "w"), indent=1)
        return
    import blsbn254_loader
    M = blsbn254_loader.load()
    eng = M.Engine(0)
    rnd = random.Random(2025)
    result = {"method": "wall: host clock around synchronous Engine calls (packing of the per-group byte strings included), %d warm-ups + %d timed "
                        "repetitions per form, alternating; spread = interquartile; kernel times from the HIP-event profile in a pass of their own" % (WARMUP, REPS),
              "shares_per_group": N_PER_GROUP, "coefficients_per_group": T, "rows": []}
    # the context's first call builds the generator table: its kernels, the table build among them, in a profile of their own
    first = make_row(eng, rnd, 16, "small", 0)
    result["first_call_kernels_ms"] = profile_of(eng, lambda: eng.threshold_verify_key_shares_batch(*first[:3]))
    result["k_g2gen_table_ms"] = result["first_call_kernels_ms"]["g2gen_table"]["ms"]
    # bring the machine and the host allocator to their steady state before the first row (discarded): both forms on an input of
    # the largest row's size for two seconds (without it the first row of a run pays page faults of fresh host buffers in both forms)
    warm = make_row(eng, rnd, 1 << 17, "small", 0)
    t_end = time.perf_counter() + 2.0
    while time.perf_counter() < t_end:
        eng.threshold_verify_key_shares_batch(*warm[:3])
        if not a.only_new:
            composition(eng, *warm[:3])
    for spec in a.rows.split(","):
        lg, kind, wrong = spec.split(":")
        n_groups, wrong = 1 << int(lg), int(wrong)
        n = n_groups * N_PER_GROUP
        commit_sets, id_sets, share_sets, want = make_row(eng, rnd, n_groups, kind, wrong)
        row = {"log2_groups": int(lg), "groups": n_groups, "shares": n, "ids": "1..7" if kind == "small" else "random in [1, r)", "wrong_every": wrong}
        new = lambda: eng.threshold_verify_key_shares_batch(commit_sets, id_sets, share_sets)
        old = lambda: composition(eng, commit_sets, id_sets, share_sets)
        assert new() == (want, bytes(n_groups)), "the new call's bitmap differs from the Python pattern"
        forms = [("new_call", new)]
        if not a.only_new:
            assert old() == (want, bytes(n_groups)), "the composition's bitmap differs from the Python pattern"
            forms.append(("composition", old))
        ts = {name: [] for name, _ in forms}
        for rep in range(WARMUP + REPS):
            for name, fn in forms:
                t0 = time.perf_counter(); fn(); dt = time.perf_counter() - t0
                if rep >= WARMUP:
                    ts[name].append(dt)
        for name, _ in forms:
            row[name] = stats(ts[name])
        ph = profile_of(eng, new)
        row["new_call_kernels_ms"] = ph
        row["k_td_key_check_ms"] = ph["td_key_check"]["ms"]
        row["k_g2_poly_eval_ms"] = ph["g2_poly_eval"]["ms"]
        if not a.only_new:
            po = profile_of(eng, old)
            row["composition_kernels_ms"] = po
            row["k_sk_to_pk_ms"] = po["sk_to_pk"]["ms"]
            row["k_td_key_check_over_k_sk_to_pk"] = round(row["k_td_key_check_ms"] / row["k_sk_to_pk_ms"], 4)
            row["new_over_composition"] = round(row["new_call"]["median_ms"] / row["composition"]["median_ms"], 3)
            row["new_below_composition_beyond_spreads"] = bool(row["new_call"]["median_ms"] + row["new_call"]["spread_ms"] + row["composition"]["spread_ms"]
                                                               < row["composition"]["median_ms"])
        print(json.dumps(row), flush=True)
        result["rows"].append(row)
    s = eng.threshold_key_check_stats()
    result["window_bits"] = s["window_bits"]
    result["table_bytes"] = (256 // s["window_bits"]) * (1 << s["window_bits"]) * 216
    result["table_builds"] = s["table_builds"]
    if not a.only_new:
        cond = [r["new_below_composition_beyond_spreads"] for r in result["rows"] if r["ids"] == "1..7" and r["log2_groups"] in (14, 17)]
        result["condition_met_on_the_short_id_rows"] = bool(cond and all(cond))
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
