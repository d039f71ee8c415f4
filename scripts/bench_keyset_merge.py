"""Checked merge of partial aggregates over a registered key set (blsbn254_keyset_merge_checked_batch) against the composition the
parent API offers on the same inputs: the host repeats the group's message per contribution,
blsbn254_keyset_fast_aggregate_verify_batch over ALL contributions (one equation each), the greedy selection of disjoint
verified contributions on the host (numpy, a step per contribution position over all groups), and a loop of
blsbn254_aggregate_sigs per group.  Both through the C ABI on numpy buffers.  The message repeat, the verify, the selection and
the loop are reported separately.
Per row: warm-up, REPS timed repetitions of each form, alternating; median, quartiles, min and max of the wall time (host clock
around calls that end synchronised).  Registration is not part of the timed call.  Kernel times come from the engine's HIP-event
profile in passes of their own, after the wall-time passes.
Usage: python scripts/bench_keyset_merge.py [--out profiles/keyset_merge.json] [--reps 20] [--rows 0,1,2,3] [--quick] -> JSON"""
import argparse, ctypes, json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import blsbn254_loader; M = blsbn254_loader.load()
from tests import synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join("profiles", "keyset_merge.json"))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rows", default="", help="comma-separated row numbers (default: all)")
ap.add_argument("--quick", action="store_true", help="tiny rows: a rehearsal of the script, not a measurement")
args = ap.parse_args()
REPS, WARM, PROF = max(args.reps, 1), 3, 2
# (groups, keys, contributions per group, keys per contribution, a wrong contribution in every k-th group or 0, name)
ROWS = [(4096, 1024, 16, 42, 0, "4096 groups, 1024 keys, 16 disjoint contributions of 42 keys, all honest"),
        (4096, 1024, 16, 42, 16, "4096 groups, 1024 keys, 16 disjoint contributions of 42 keys, one wrong contribution in every 16th group"),
        (4096, 64, 8, 8, 0, "4096 groups, 64 keys, 8 contributions of 8 keys"), (16, 64, 8, 8, 0, "16 groups, 64 keys, 8 contributions of 8 keys")]
if args.quick:
    ROWS = [(24, 70, 4, 9, 0, "quick honest"), (24, 70, 4, 9, 4, "quick one wrong in every 4th"), (16, 64, 8, 8, 0, "quick all")]
if args.rows:
    ROWS = [ROWS[int(k)] for k in args.rows.split(",")]
u8, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
P8 = lambda a: a.ctypes.data_as(u8)
P64 = lambda a: a.ctypes.data_as(u64)
dst = M.DEFAULT_DST
e = M.Engine(0)
lib, ctx = e._lib, e._ctx
R = synth.R
NMAX = max(r[1] for r in ROWS)
sk_int = [int(synth.sk_of(k)) for k in range(NMAX)]
pk_all = np.frombuffer(e.sk_to_pk_batch(b"".join(s.to_bytes(32, "big") for s in sk_int), NMAX), dtype=np.uint8).reshape(NMAX, 128)
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
for G, n, C, K, wrong_every, name in ROWS:
    pks = np.ascontiguousarray(pk_all[:n])
    rb, N = (n + 7) // 8, G * C
    # contribution c of every group: the keys c K .. (c + 1) K, signed by the sum of their secrets on the group's message; a wrong
    # one (contribution 1 of every wrong_every-th group) by that sum + 1
    cbits = np.zeros((C, n), dtype=bool)
    for c in range(C):
        cbits[c, c * K:(c + 1) * K] = True
    crows = np.packbits(cbits, axis=1, bitorder="little")               # (C, rb)
    rows = np.ascontiguousarray(np.tile(crows, (G, 1)))                 # (N, rb)
    csk = [sum(sk_int[c * K:(c + 1) * K]) % R for c in range(C)]
    sk_tab = np.frombuffer(b"".join((s or 1).to_bytes(32, "big") for s in csk + [(s + 1) % R or 1 for s in csk]), dtype=np.uint8).reshape(2 * C, 32)
    grp = np.repeat(np.arange(G), C)
    signer = np.tile(np.arange(C), G)
    bad = np.array([g * C + 1 for g in range(0, G, wrong_every)] if wrong_every else [], dtype=np.int64)
    signer[bad] += C
    msg_tab = np.frombuffer(b"".join(synth.msg_of(80000 + g) for g in range(G)), dtype=np.uint8).reshape(G, ML)
    moff = (np.arange(G + 1, dtype=np.uint64) * ML)
    emoff = (np.arange(N + 1, dtype=np.uint64) * ML)
    coff = (np.arange(G + 1, dtype=np.uint64) * C)
    sigs = np.zeros(64 * N, dtype=np.uint8)
    sk = np.ascontiguousarray(sk_tab[signer]); em = np.ascontiguousarray(msg_tab[grp])
    assert lib.blsbn254_sign_batch(ctx, P8(sk), P8(em), P64(emoff), ctypes.c_size_t(N), dst, ctypes.c_size_t(len(dst)), P8(sigs)) == 0
    want_used = np.ones(N, dtype=bool); want_used[bad] = False
    want_rows = np.zeros((G, rb), dtype=np.uint8)
    for c in range(C):
        want_rows |= crows[c][None, :] * want_used.reshape(G, C)[:, c][:, None].astype(np.uint8)
    h = ctypes.c_void_p()
    assert lib.blsbn254_keyset_create(ctx, P8(pks), ctypes.c_size_t(n), ctypes.byref(h)) == 0
    o_new, r_new, s_new = np.zeros(64 * G, dtype=np.uint8), np.zeros(rb * G, dtype=np.uint8), np.zeros(G, dtype=np.uint8)
    u_new = np.zeros((N + 7) // 8, dtype=np.uint8)
    o_old, r_old = np.zeros(64 * G, dtype=np.uint8), np.zeros((G, rb), dtype=np.uint8)
    u_old = np.zeros(N, dtype=bool)
    vbm = np.zeros((N + 7) // 8 + 1, dtype=np.uint8)
    rows3 = rows.reshape(G, C, rb)

    def run_new():
        t = time.perf_counter()
        rc = lib.blsbn254_keyset_merge_checked_batch(ctx, h, P8(rows), P8(sigs), P64(coff), P8(msg_tab), P64(moff), ctypes.c_size_t(G), dst,
                                                     ctypes.c_size_t(len(dst)), P8(o_new), P8(r_new), P8(u_new), P8(s_new))
        dt = time.perf_counter() - t
        assert rc == 0
        return dt * 1e3, 0.0, 0.0, 0.0, 0.0

    def run_old():
        t = time.perf_counter()
        emsgs = msg_tab[grp]                                            # the message per contribution
        tg = time.perf_counter()
        rc = lib.blsbn254_keyset_fast_aggregate_verify_batch(ctx, h, P8(rows), P8(emsgs), P64(emoff), P8(sigs), ctypes.c_size_t(N), dst, ctypes.c_size_t(len(dst)),
                                                             P8(vbm))
        assert rc == 0
        tv = time.perf_counter()
        good = np.unpackbits(vbm, count=N, bitorder="little").astype(bool).reshape(G, C)      # the greedy selection, in order
        union = np.zeros((G, rb), dtype=np.uint8)
        take = np.zeros((G, C), dtype=bool)
        for c in range(C):
            r = rows3[:, c]
            ok = good[:, c] & ~(r & union).any(axis=1)
            union |= r * ok[:, None].astype(np.uint8)
            take[:, c] = ok
        r_old[:] = union; u_old[:] = take.reshape(N)
        keep = np.nonzero(u_old)[0]
        cnt = take.sum(axis=1)
        koff = np.concatenate([[0], np.cumsum(cnt)])
        ksig = np.ascontiguousarray(sigs.reshape(N, 64)[keep])
        ts = time.perf_counter()
        for g in range(G):
            rc = lib.blsbn254_aggregate_sigs(ctx, P8(ksig[koff[g]:]), ctypes.c_size_t(int(cnt[g])), P8(o_old[64 * g:]))
            assert rc == 0
        te = time.perf_counter()
        return (te - t) * 1e3, (tg - t) * 1e3, (tv - tg) * 1e3, (ts - tv) * 1e3, (te - ts) * 1e3

    for _ in range(WARM):
        run_new(); run_old()
    assert s_new.tobytes() == bytes(G) and r_new.tobytes() == want_rows.tobytes() == r_old.tobytes() and o_new.tobytes() == o_old.tobytes(), name
    assert np.array_equal(np.unpackbits(u_new, count=N, bitorder="little").astype(bool), want_used) and np.array_equal(u_old, want_used), name
    t_new, t_old, t_parts = [], [], []
    for _ in range(REPS):
        t_new.append(run_new()[0])
        o = run_old(); t_old.append(o[0]); t_parts.append(o[1:])
    ms = (ctypes.c_uint64 * 4)(); lib.blsbn254_keyset_merge_stats(ctx, ms)
    parts = np.median(np.array(t_parts), axis=0)
    row = {"groups": G, "keys": n, "contributions": int(N), "wrong_contributions": int(len(bad)), "merge_stats_since_start": [int(x) for x in ms],
           "checked": stats(t_new), "composition": stats(t_old),
           "composition_median_ms": {"message_repeat": round(float(parts[0]), 3), "keyset_fast_aggregate_verify_batch": round(float(parts[1]), 3),
                                     "host_selection": round(float(parts[2]), 3), "aggregate_sigs_loop": round(float(parts[3]), 3)}}
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
