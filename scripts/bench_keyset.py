"""FastAggregateVerify over a registered key set by bitmaps (blsbn254_keyset_fast_aggregate_verify_batch) against the composition the
parent API offers on the same inputs: the host gathers the selected keys from the bitmaps (one numpy take, counted in the wall
time: a caller has to do it) and calls blsbn254_fast_aggregate_verify_batch.  Both through the C ABI on numpy buffers.
Per row: warm-up, REPS timed repetitions of each form, alternating; median, quartiles, min and max of the wall time (host clock
around calls that end synchronised).  Registration is timed separately and is not part of the timed call.  Kernel times come from
the engine's HIP-event profile in passes of their own, after the wall-time passes.
Usage: python scripts/bench_keyset.py [--out profiles/keyset.json] [--reps 20] [--quick] -> JSON"""
import argparse, ctypes, json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import blsbn254_loader; M = blsbn254_loader.load()
from tests import synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join("profiles", "keyset.json"))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--quick", action="store_true", help="tiny rows: a rehearsal of the script, not a measurement")
args = ap.parse_args()
REPS, WARM, PROF = max(args.reps, 1), 3, 3
ROWS = [(4096, 1024, 2 / 3, "4096 groups, 1024 keys, 2/3 participation"), (4096, 1024, 1 / 3, "4096 groups, 1024 keys, 1/3 participation (no complement)"),
        (4096, 64, 1.0, "4096 groups, 64 keys, all selected"), (16, 64, 1.0, "16 groups, 64 keys, all selected")]
if args.quick:
    ROWS = [(24, 70, 2 / 3, "quick 2/3"), (24, 70, 1 / 3, "quick 1/3"), (24, 64, 1.0, "quick all")]
u8, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
P8 = lambda a: a.ctypes.data_as(u8)
dst = M.DEFAULT_DST
e = M.Engine(0)
lib, ctx = e._lib, e._ctx
R = synth.R
NMAX = max(r[1] for r in ROWS)
sks = np.array([synth.sk_of(k) for k in range(NMAX)], dtype=object)
pk_all = np.frombuffer(e.sk_to_pk_batch(b"".join(int(s).to_bytes(32, "big") for s in sks), NMAX), dtype=np.uint8).reshape(NMAX, 128)


def stats(ms):
    a = np.sort(np.array(ms))
    q1, med, q3 = (float(np.percentile(a, p)) for p in (25, 50, 75))
    return {"median_ms": round(med, 3), "spread_ms": round(q3 - q1, 3), "q1_ms": round(q1, 3), "q3_ms": round(q3, 3), "min_ms": round(float(a[0]), 3),
            "max_ms": round(float(a[-1]), 3), "reps": len(ms)}


def kernels(reps):
    pr = e.profile_read()
    return {n: round(v["total_ms"] / reps, 3) for n, v in sorted(pr.items()) if v["total_ms"] / reps > 0.005}


out = {"method": "wall: host clock around C-ABI calls that end synchronised, %d warm-up + %d timed repetitions per form, alternating; spread = interquartile "
                 "range; kernel_ms: HIP-event profile, mean of %d further repetitions in passes of their own" % (WARM, REPS, PROF), "rows": {}}
rnd = np.random.RandomState(7)
for G, n, part, name in ROWS:
    pks = np.ascontiguousarray(pk_all[:n])
    bits = np.ones((G, n), dtype=bool) if part >= 1.0 else rnd.random_sample((G, n)) < part
    bits[:, 0] = True
    sel = np.packbits(bits, axis=1, bitorder="little")                 # G rows of ceil(n / 8) bytes, LSB-first
    assert sel.shape == (G, (n + 7) // 8)
    agg = [int(sum(sks[:n][bits[g]])) % R or 1 for g in range(G)]
    msgs = [synth.msg_of(50000 + g) for g in range(G)]
    sigs = np.frombuffer(e.sign_batch(b"".join(s.to_bytes(32, "big") for s in agg), msgs, dst), dtype=np.uint8)
    for g in range(6, G, 7):
        msgs[g] = bytes([msgs[g][0] ^ 1]) + msgs[g][1:]
    want = synth.bitmap_of([g % 7 != 6 for g in range(G)])
    data, off = M.engine.pack_messages(msgs)
    data = np.frombuffer(data, dtype=np.uint8)
    nb = (G + 7) // 8
    bm_new, bm_old = np.zeros(nb, dtype=np.uint8), np.zeros(nb, dtype=np.uint8)
    t0 = time.perf_counter()
    h = ctypes.c_void_p()
    assert lib.blsbn254_keyset_create(ctx, P8(pks), ctypes.c_size_t(n), ctypes.byref(h)) == 0
    reg_ms = (time.perf_counter() - t0) * 1e3

    def run_new():
        t = time.perf_counter()
        rc = lib.blsbn254_keyset_fast_aggregate_verify_batch(ctx, h, P8(sel), P8(data), off.ctypes.data_as(u64), P8(sigs), ctypes.c_size_t(G), dst,
                                                             ctypes.c_size_t(len(dst)), P8(bm_new))
        dt = time.perf_counter() - t
        assert rc == 0
        return dt * 1e3, 0.0

    def run_old():
        t = time.perf_counter()
        rows, cols = np.nonzero(np.unpackbits(sel, axis=1, count=n, bitorder="little"))      # the gather a caller of the parent API does
        koff = np.zeros(G + 1, dtype=np.uint64)
        koff[1:] = np.cumsum(np.bincount(rows, minlength=G))
        gathered = pks[cols]
        tg = time.perf_counter()
        rc = lib.blsbn254_fast_aggregate_verify_batch(ctx, P8(gathered), koff.ctypes.data_as(u64), P8(data), off.ctypes.data_as(u64), P8(sigs),
                                                      ctypes.c_size_t(G), dst, ctypes.c_size_t(len(dst)), P8(bm_old))
        dt = time.perf_counter() - t
        assert rc == 0
        return dt * 1e3, (tg - t) * 1e3

    for _ in range(WARM):
        run_new(); run_old()
    assert bm_new.tobytes() == want and bm_old.tobytes() == want, name
    t_new, t_old, t_gather = [], [], []
    for _ in range(REPS):
        t_new.append(run_new()[0])
        o = run_old(); t_old.append(o[0]); t_gather.append(o[1])
    row = {"groups": G, "keys": n, "selected_keys": int(bits.sum()), "registration_ms": round(reg_ms, 3), "keyset": stats(t_new), "composition": stats(t_old),
           "composition_gather_median_ms": round(float(np.median(t_gather)), 3)}
    e.profile_enable(True)
    for key, fn in (("keyset", run_new), ("composition", run_old)):
        e.profile_reset()
        for _ in range(PROF):
            fn()
        row[key]["kernel_ms"] = kernels(PROF)
    e.profile_enable(False); e.profile_reset()
    kn, kc = row["keyset"]["kernel_ms"], row["composition"]["kernel_ms"]
    row["sum_kernels_ms"] = {"keyset: ks_word_sum + ks_group_sum": round(kn.get("ks_word_sum", 0) + kn.get("ks_group_sum", 0), 3),
                             "composition: g2_load + g2_seg_sum": round(kc.get("g2_load", 0) + kc.get("g2_seg_sum", 0), 3)}
    a, b = row["keyset"], row["composition"]
    row["wall_condition_met"] = bool(a["median_ms"] + a["spread_ms"] + b["spread_ms"] < b["median_ms"])
    out["rows"][name] = row
    lib.blsbn254_keyset_destroy(h)
e.close()
text = json.dumps(out, indent=1)
os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
open(args.out, "w").write(text + "\n")
print(text)
