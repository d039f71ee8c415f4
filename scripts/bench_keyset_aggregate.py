"""Checked signature aggregation over a registered key set (blsbn254_keyset_aggregate_checked_batch) against the composition the
parent API offers on the same inputs: the host gathers the signers' keys (one numpy take) and repeats the group's message per
entry, blsbn254_verify_batch over all entries, the host selection of the good ones, and a loop of blsbn254_aggregate_sigs per
group.  Both through the C ABI on numpy buffers.  The gather, the verify and the loop are reported separately.
Per row: warm-up, REPS timed repetitions of each form, alternating; median, quartiles, min and max of the wall time (host clock
around calls that end synchronised).  Registration is not part of the timed call.  Kernel times come from the engine's HIP-event
profile in passes of their own, after the wall-time passes.
Usage: python scripts/bench_keyset_aggregate.py [--out profiles/keyset_aggregate.json] [--reps 20] [--rows 0,1,2,3] [--quick] -> JSON"""
import argparse, ctypes, json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import blsbn254_loader; M = blsbn254_loader.load()
from tests import synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join("profiles", "keyset_aggregate.json"))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rows", default="", help="comma-separated row numbers (default: all)")
ap.add_argument("--quick", action="store_true", help="tiny rows: a rehearsal of the script, not a measurement")
args = ap.parse_args()
REPS, WARM, PROF = max(args.reps, 1), 3, 2
# (groups, keys, participation, a wrong signature in every k-th group or 0, name)
ROWS = [(4096, 1024, 2 / 3, 0, "4096 groups, 1024 keys, 2/3 participation, all honest"),
        (4096, 1024, 2 / 3, 16, "4096 groups, 1024 keys, 2/3 participation, one wrong signature in every 16th group"),
        (4096, 64, 1.0, 0, "4096 groups, 64 keys, all signing"), (16, 64, 1.0, 0, "16 groups, 64 keys, all signing")]
if args.quick:
    ROWS = [(24, 70, 2 / 3, 0, "quick honest"), (24, 70, 2 / 3, 4, "quick one wrong in every 4th"), (16, 64, 1.0, 0, "quick all")]
if args.rows:
    ROWS = [ROWS[int(k)] for k in args.rows.split(",")]
u8, u32, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
P8 = lambda a: a.ctypes.data_as(u8)
P64 = lambda a: a.ctypes.data_as(u64)
dst = M.DEFAULT_DST
e = M.Engine(0)
lib, ctx = e._lib, e._ctx
R = synth.R
NMAX = max(r[1] for r in ROWS)
sk_all = np.frombuffer(b"".join(int(synth.sk_of(k)).to_bytes(32, "big") for k in range(NMAX + 1)), dtype=np.uint8).reshape(NMAX + 1, 32)
pk_all = np.frombuffer(e.sk_to_pk_batch(sk_all[:NMAX].tobytes(), NMAX), dtype=np.uint8).reshape(NMAX, 128)
ML = 32                                                                # message length (synth.msg_of)


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
rnd = np.random.RandomState(9)
for G, n, part, wrong_every, name in ROWS:
    pks = np.ascontiguousarray(pk_all[:n])
    bits = np.ones((G, n), dtype=bool) if part >= 1.0 else rnd.random_sample((G, n)) < part
    bits[:, 0] = True
    grp, idx = np.nonzero(bits)                                         # entries in group order, indices increasing inside a group
    idx = idx.astype(np.uint32)
    N = len(idx)
    soff = np.zeros(G + 1, dtype=np.uint64)
    soff[1:] = np.cumsum(np.bincount(grp, minlength=G))
    msg_tab = np.frombuffer(b"".join(synth.msg_of(70000 + g) for g in range(G)), dtype=np.uint8).reshape(G, ML)
    moff = (np.arange(G + 1, dtype=np.uint64) * ML)
    emoff = (np.arange(N + 1, dtype=np.uint64) * ML)
    # every entry signed by its key on its group's message; the wrong ones by the next key of the sequence
    signer = idx.astype(np.int64)
    bad_entries = np.array([int(soff[g]) + 1 for g in range(0, G, wrong_every)] if wrong_every else [], dtype=np.int64)
    signer[bad_entries] += 1
    sigs = np.zeros(64 * N, dtype=np.uint8)
    STEP = 1 << 19
    for lo in range(0, N, STEP):                                        # (by pieces: the per-entry messages are built on the host)
        hi = min(N, lo + STEP)
        sk = np.ascontiguousarray(sk_all[signer[lo:hi]]); em = np.ascontiguousarray(msg_tab[grp[lo:hi]])
        assert lib.blsbn254_sign_batch(ctx, P8(sk), P8(em), P64(emoff), ctypes.c_size_t(hi - lo), dst, ctypes.c_size_t(len(dst)), P8(sigs[64 * lo:])) == 0
    rb = (n + 7) // 8
    want_bits = bits.copy()
    want_bits[grp[bad_entries], idx[bad_entries]] = False
    want_rows = np.packbits(want_bits, axis=1, bitorder="little")
    h = ctypes.c_void_p()
    assert lib.blsbn254_keyset_create(ctx, P8(pks), ctypes.c_size_t(n), ctypes.byref(h)) == 0
    o_new, r_new, s_new = np.zeros(64 * G, dtype=np.uint8), np.zeros(rb * G, dtype=np.uint8), np.zeros(G, dtype=np.uint8)
    o_old, r_old = np.zeros(64 * G, dtype=np.uint8), np.zeros((G, rb), dtype=np.uint8)
    vbm = np.zeros((N + 7) // 8 + 1, dtype=np.uint8)

    def run_new():
        t = time.perf_counter()
        rc = lib.blsbn254_keyset_aggregate_checked_batch(ctx, h, idx.ctypes.data_as(u32), P8(sigs), P64(soff), P8(msg_tab), P64(moff), ctypes.c_size_t(G), dst,
                                                         ctypes.c_size_t(len(dst)), P8(o_new), P8(r_new), P8(s_new))
        dt = time.perf_counter() - t
        assert rc == 0
        return dt * 1e3, 0.0, 0.0, 0.0

    def run_old():
        t = time.perf_counter()
        gathered = pks[idx]                                             # the gather a caller of the parent API does, and the message per entry
        emsgs = msg_tab[grp]
        tg = time.perf_counter()
        rc = lib.blsbn254_verify_batch(ctx, P8(gathered), P8(emsgs), P64(emoff), P8(sigs), ctypes.c_size_t(N), dst, ctypes.c_size_t(len(dst)), P8(vbm))
        assert rc == 0
        tv = time.perf_counter()
        good = np.unpackbits(vbm, count=N, bitorder="little").astype(bool)      # the selection, and the rows
        keep = np.nonzero(good)[0]
        cnt = np.bincount(grp[keep], minlength=G)
        koff = np.concatenate([[0], np.cumsum(cnt)])
        ksig = np.ascontiguousarray(sigs.reshape(N, 64)[keep])
        sel = np.zeros((G, n), dtype=bool); sel[grp[keep], idx[keep]] = True
        r_old[:] = np.packbits(sel, axis=1, bitorder="little")
        ts = time.perf_counter()
        for g in range(G):
            rc = lib.blsbn254_aggregate_sigs(ctx, P8(ksig[koff[g]:]), ctypes.c_size_t(int(cnt[g])), P8(o_old[64 * g:]))
            assert rc == 0
        te = time.perf_counter()
        return (te - t) * 1e3, (tg - t) * 1e3, (tv - tg) * 1e3, (te - ts) * 1e3

    for _ in range(WARM):
        run_new(); run_old()
    assert s_new.tobytes() == bytes(G) and r_new.tobytes() == want_rows.tobytes() == r_old.tobytes() and o_new.tobytes() == o_old.tobytes(), name
    t_new, t_old, t_parts = [], [], []
    for _ in range(REPS):
        t_new.append(run_new()[0])
        o = run_old(); t_old.append(o[0]); t_parts.append(o[1:])
    ag = (ctypes.c_uint64 * 4)(); lib.blsbn254_keyset_aggregate_stats(ctx, ag)
    parts = np.median(np.array(t_parts), axis=0)
    row = {"groups": G, "keys": n, "entries": int(N), "wrong_signatures": int(len(bad_entries)), "checked": stats(t_new), "composition": stats(t_old),
           "composition_median_ms": {"gather": round(float(parts[0]), 3), "verify_batch": round(float(parts[1]), 3), "aggregate_sigs_loop": round(float(parts[2]), 3)}}
    e.profile_enable(True)
    for key, fn in (("checked", run_new), ("composition", run_old)):
        e.profile_reset()
        for _ in range(PROF):
            fn()
        row[key]["kernel_ms"] = kernels(PROF)
    e.profile_enable(False); e.profile_reset()
    a, b = row["checked"], row["composition"]
    row["wall_condition_met"] = bool(a["median_ms"] + a["spread_ms"] + b["spread_ms"] < b["median_ms"])
    out["rows"][name] = row
    lib.blsbn254_keyset_destroy(h)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    open(args.out, "w").write(json.dumps(out, indent=1) + "\n")          # after every row: a run that is cut short keeps what it measured
    print(name, json.dumps(row), flush=True)
e.close()
print(json.dumps(out, indent=1))
