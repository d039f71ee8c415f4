"""Aggregate verify over groups of (key, message) pairs (blsbn254_aggregate_verify_batch) on one GPU, against what a caller had
before it: the host composition hash_to_g1_batch + interleave (sig, -G2gen) with the (H(msg_i), pk_i) pairs + pairing_check_batch
+ g1_check_batch / identity tests of the signatures and keys, and (at 2^10 groups) the loop of aggregate_verify calls.

The composition and the loop only use entry points the parent commit has, and are to be measured on the PARENT commit's build:
    BLSBN254_LIB=<parent build>.so python scripts/bench_aggregate_batch.py --phase parent --out parent.json
    python scripts/bench_aggregate_batch.py --phase fused --parent parent.json --out profiles/aggregate_batch.json
The second run measures the fused call on this build (host clock around the synchronous call, min of --reps repetitions after
one warm-up, max - min recorded as the spread), its per-kernel times from the engine's HIP-event profile, merges the parent
rows and states per row whether fused < composition by more than the two spreads combined.  Groups are cut from one batch of
unique signed tuples over a 1024-key pool; every 16th group has one message flipped; every path must give that bitmap."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
IDENT1_X = bytes(32)
IDENT2_X = bytes(64)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return 1e3 * min(ts), 1e3 * (max(ts) - min(ts))


def groups_of(O, batch, n_g, k):
    """the first n_g * k tuples as n_g groups of k: flat keys, message list, aggregate signatures, expected bitmap"""
    pks, msgs, sigs = batch
    n = n_g * k
    msgs = list(msgs[:n])
    if k == 1:
        aggs = sigs[:64 * n]
    else:
        aggs = b"".join(O.aggregate_sigs(sigs[64 * k * g:64 * k * (g + 1)], k) for g in range(n_g))
    want = np.ones(n_g, dtype=np.uint8)
    for g in range(15, n_g, 16):
        i = k * g + (g // 16) % k
        msgs[i] = bytes([msgs[i][0] ^ 1]) + msgs[i][1:]
        want[g] = 0
    return pks[:128 * n], msgs, aggs, np.packbits(want, bitorder="little").tobytes()


def composition(eng, neg_g2, pks, msgs, aggs, n_g, k, dst):
    """what a caller composes from the parent's entry points; the pairing check allows identity members, aggregate verify does not"""
    n = n_g * k
    H = np.frombuffer(eng.hash_to_g1_batch(msgs, dst), dtype=np.uint8).reshape(n_g, k * 64)
    S = np.frombuffer(aggs, dtype=np.uint8).reshape(n_g, 64)
    K = np.frombuffer(pks, dtype=np.uint8).reshape(n_g, k * 128)
    P = np.concatenate([S, H], axis=1).tobytes()
    Q = np.concatenate([np.broadcast_to(np.frombuffer(neg_g2, dtype=np.uint8), (n_g, 128)), K], axis=1).tobytes()
    off = np.arange(0, n_g * (k + 1) + 1, k + 1, dtype=np.uint64)
    bits = np.unpackbits(np.frombuffer(eng.pairing_check_batch(P, Q, off), dtype=np.uint8), bitorder="little")[:n_g]
    sig_ok = np.unpackbits(np.frombuffer(eng.g1_check_batch(aggs, n_g), dtype=np.uint8), bitorder="little")[:n_g]
    sig_id = ~S[:, :32].any(axis=1)
    key_id = ~np.frombuffer(pks, dtype=np.uint8).reshape(n, 128)[:, :64].any(axis=1)
    ok = bits.astype(bool) & sig_ok.astype(bool) & ~sig_id & ~key_id.reshape(n_g, k).any(axis=1)
    return np.packbits(ok.astype(np.uint8), bitorder="little").tobytes()


def loop_single(eng, pks, msgs, aggs, n_g, k, dst):
    out = [eng.aggregate_verify(pks[128 * k * g:128 * k * (g + 1)], msgs[k * g:k * (g + 1)], aggs[64 * g:64 * g + 64], dst) for g in range(n_g)]
    return np.packbits(np.array(out, dtype=np.uint8), bitorder="little").tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", choices=["parent", "fused"], required=True)
    ap.add_argument("--parent", default=None, help="the JSON written by --phase parent (merged by --phase fused)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="10x4,14x4,16x4,18x1,12x64", help="log2(groups) x pairs per group")
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
    pks, msgs, sigs, _ = synth.make_batch_gpu(eng, O, n_max, dst, pool=1024, invalid_every=0, spot=16)
    pks, sigs = bytes(pks), bytes(sigs)
    neg_g2 = O.g2_mul(O.g2_generator(), R - 1)
    parent = {}
    if a.phase == "fused" and a.parent:
        parent = {(r["groups"], r["pairs_per_group"]): r for r in json.load(open(a.parent))["rows"]}
    rows = []
    for lg, k in shapes:
        n_g = 1 << lg
        gp, gm, ga, want = groups_of(O, (pks, msgs, sigs), n_g, k)
        row = {"log2_groups": lg, "groups": n_g, "pairs_per_group": k, "pairs": n_g * k}
        if a.phase == "parent":
            assert composition(eng, neg_g2, gp, gm, ga, n_g, k, dst) == want, "the composition's bitmap differs from the closed form"
            t, sp = timed(lambda: composition(eng, neg_g2, gp, gm, ga, n_g, k, dst), a.reps)
            row.update({"composition_ms": round(t, 3), "composition_spread_ms": round(sp, 3)})
            if lg == 10:
                assert loop_single(eng, gp, gm, ga, n_g, k, dst) == want
                t, sp = timed(lambda: loop_single(eng, gp, gm, ga, n_g, k, dst), a.reps)
                row.update({"single_call_loop_ms": round(t, 3), "single_call_loop_spread_ms": round(sp, 3)})
        else:
            key_sets = [gp[128 * k * g:128 * k * (g + 1)] for g in range(n_g)]
            msg_sets = [gm[k * g:k * (g + 1)] for g in range(n_g)]
            goff = np.arange(0, n_g * k + 1, k, dtype=np.uint64)
            assert eng.aggregate_verify_batch(key_sets, msg_sets, ga, dst) == want, "the fused bitmap differs from the closed form"
            t, sp = timed(lambda: eng.aggregate_verify_batch_flat(gp, gm, goff, ga, dst), a.reps)
            eng.profile_reset(); eng.profile_enable(True)
            eng.aggregate_verify_batch_flat(gp, gm, goff, ga, dst)
            eng.profile_enable(False)
            phases = {name: {"launches": v["launches"], "ms": round(v["total_ms"], 3)} for name, v in eng.profile_read().items()}
            lanes = n_g * ((k + 2) // 2)
            row.update({"fused_ms": round(t, 3), "fused_spread_ms": round(sp, 3), "groups_per_s": round(n_g / (t / 1e3)),
                        "kernel_phases_ms": phases, "kernel_total_ms": round(sum(v["ms"] for v in phases.values()), 3),
                        "two_pair_lanes": lanes,
                        "miller_hpk2r_us_per_pair": round(1e3 * phases["miller_hpk2r"]["ms"] / (n_g * (k + 1)), 5)})
            p = parent.get((n_g, k))
            if p:
                row.update({x: p[x] for x in p if x.startswith(("composition", "single_call"))})
                margin = row["fused_spread_ms"] + p["composition_spread_ms"]
                row["fused_over_composition"] = round(t / p["composition_ms"], 3)
                row["speedup"] = round(p["composition_ms"] / t, 2)
                row["faster_than_composition_beyond_spread"] = bool(p["composition_ms"] - t > margin)
        print(json.dumps(row), flush=True)
        rows.append(row)
    small = None
    if a.phase == "fused":
        # a call far too small to fill the chip (16 groups of 4): no latency form is wired in, so it costs one lane's chain
        gp, gm, ga, want = groups_of(O, (pks, msgs, sigs), 16, 4)
        goff = np.arange(0, 65, 4, dtype=np.uint64)
        assert eng.aggregate_verify_batch_flat(gp, gm, goff, ga, dst) == want
        t, sp = timed(lambda: eng.aggregate_verify_batch_flat(gp, gm, goff, ga, dst), a.reps)
        small = {"groups": 16, "pairs_per_group": 4, "fused_ms": round(t, 3), "fused_spread_ms": round(sp, 3)}
        print(json.dumps({"small_call": small}), flush=True)
        row_stats = eng.aggregate_batch_stats()
        print(json.dumps({"stats": row_stats}), flush=True)
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"composition": "hash_to_g1_batch + host interleave of (sig, -G2gen) with the (H(msg_i), pk_i) pairs + pairing_check_batch + g1_check_batch "
                                      "and identity tests on the host; measured on the parent commit's build, as is the loop of aggregate_verify calls",
                       "timing": "host clock around the synchronous call, min of reps after one warm-up; spread = max - min of the reps",
                       "reps": a.reps, "phase": a.phase, "rows": rows, **({"small_call": small} if small else {})}, f, indent=1)


if __name__ == "__main__":
    main()
