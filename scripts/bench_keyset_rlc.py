"""FastAggregateVerify over a registered key set by random linear combination per message
(blsbn254_keyset_fast_aggregate_verify_batch_rlc and its committee form) against the EXACT call of the parent on identical inputs
(blsbn254_keyset_fast_aggregate_verify_batch / blsbn254_keyset_committee_fast_aggregate_verify_batch).  All through the C ABI on
numpy buffers.  Per row: warm-up, REPS timed repetitions of each form, alternating; median, quartiles, min and max of the wall
time (host clock around calls that end synchronised).  Kernel times come from the engine's HIP-event profile in passes of their
own.  The new call runs with seed = NULL, the production setting.  Both forms are checked to give the expected bitmap.
Usage: python scripts/bench_keyset_rlc.py [--out profiles/keyset_rlc.json] [--reps 20] [--only 0,2] [--quick] -> JSON
(--only: row numbers; the rows of an existing --out file are kept)"""
import argparse, ctypes, json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import blsbn254_loader; M = blsbn254_loader.load()
from tests import synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join("profiles", "keyset_rlc.json"))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--only", default="")
ap.add_argument("--quick", action="store_true", help="tiny rows: a rehearsal of the script, not a measurement")
args = ap.parse_args()
REPS, WARM, PROF = max(args.reps, 1), 3, 3
C = 64                                                                   # the default chunk
# registry keys, committees (0: the full-width form), members each, groups per committee (full-width: groups), message of group g,
# wrong signature in every k-th chunk (0: none), name
ROWS = [(1024, 0, 1024, 4096, lambda g, c: 0, 0, "4096 groups x 1024 keys at 2/3, ONE message"),
        (1024, 0, 1024, 4096, lambda g, c: g % 64, 0, "4096 groups x 1024 keys at 2/3, 64 messages"),
        (1024, 0, 1024, 4096, lambda g, c: g, 0, "4096 groups x 1024 keys at 2/3, all messages distinct"),
        (65536, 2048, 32, 16, lambda g, c: c // 64, 0, "32768 groups over 2048 committees of 32, one message per 64 committees"),
        (1024, 0, 1024, 4096, lambda g, c: 0, 16, "4096 groups x 1024 keys at 2/3, ONE message, a wrong signature in every 16th chunk")]
if args.quick:
    ROWS = [(70, 0, 70, 150, lambda g, c: g % 2, 2, "quick full-width"), (700, 10, 70, 13, lambda g, c: c // 5, 0, "quick committees")]
only = [int(t) for t in args.only.split(",") if t] or list(range(len(ROWS)))
u8, u32, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
P8 = lambda a: a.ctypes.data_as(u8)
P32 = lambda a: a.ctypes.data_as(u32)
P64 = lambda a: a.ctypes.data_as(u64)
SZ = ctypes.c_size_t
NOSEED = ctypes.cast(None, u8)
dst = M.DEFAULT_DST
e = M.Engine(0)
lib, ctx = e._lib, e._ctx
R = synth.R
NMAX = max(ROWS[i][0] for i in only)
sks = np.array([synth.sk_of(k) for k in range(NMAX)], dtype=object)
pk_all = np.frombuffer(e.sk_to_pk_batch(b"".join(int(s).to_bytes(32, "big") for s in sks), NMAX), dtype=np.uint8).reshape(NMAX, 128)


def stats(ms):
    a = np.sort(np.array(ms))
    q1, med, q3 = (float(np.percentile(a, p)) for p in (25, 50, 75))
    return {"median_ms": round(med, 3), "spread_ms": round(q3 - q1, 3), "q1_ms": round(q1, 3), "q3_ms": round(q3, 3), "min_ms": round(float(a[0]), 3),
            "max_ms": round(float(a[-1]), 3), "reps": len(ms)}


def kernels(reps):
    pr = e.profile_read()
    return {n: round(v["total_ms"] / reps, 4) for n, v in sorted(pr.items()) if v["total_ms"] / reps > 0.002}


def below(a, b):
    """the condition of DESIGN.md 6h: a's median lies below b's by more than the two spreads together"""
    return bool(a["median_ms"] + a["spread_ms"] + b["spread_ms"] < b["median_ms"])


def rlc_stats():
    o = (ctypes.c_uint64 * 6)()
    assert lib.blsbn254_keyset_rlc_stats(ctx, o) == 0
    return [int(x) for x in o]


out = {"method": "wall: host clock around C-ABI calls that end synchronised, %d warm-up + %d timed repetitions per form, alternating; spread = interquartile "
                 "range; kernel_ms: HIP-event profile, mean of %d further repetitions in passes of their own; the new call with seed = NULL" % (WARM, REPS, PROF),
       "rows": {}}
if args.only and os.path.exists(args.out):
    out["rows"] = json.load(open(args.out)).get("rows", {})
rnd = np.random.RandomState(13)
for ri in only:
    n, n_com, size, per, msg_id, wrong_every, name = ROWS[ri]
    committee = n_com > 0
    G = n_com * per if committee else per
    pks = np.ascontiguousarray(pk_all[:n])
    com = np.repeat(np.arange(max(n_com, 1), dtype=np.uint32), per if committee else G)[:G]
    bits = rnd.random_sample((G, size)) < 2 / 3
    bits[:, 0] = True
    rows = np.packbits(bits, axis=1, bitorder="little")                 # G rows of ceil(size / 8) bytes, LSB-first
    sel_off = np.arange(G + 1, dtype=np.uint64) * np.uint64(rows.shape[1])
    sk_mat = sks[:max(n_com, 1) * size].reshape(max(n_com, 1), size)    # committee c = keys [c size, (c + 1) size)
    agg = [int(sum(sk_mat[com[g]][bits[g]])) % R or 1 for g in range(G)]
    ids = [msg_id(g, int(com[g])) for g in range(G)]
    msgs = [synth.msg_of(80000 + i) for i in ids]
    # the chunks of the plan: a class in the caller's order, cut into runs of C
    seen, wrong = {}, []
    for g, i in enumerate(ids):
        k = seen.get(i, 0)
        seen[i] = k + 1
        if wrong_every and k % C == 5 and (k // C) % wrong_every == 0:
            wrong.append(g)
    signed = list(msgs)
    for g in wrong:
        signed[g] = b"not the message of this group"
    sigs = np.frombuffer(e.sign_batch(b"".join(s.to_bytes(32, "big") for s in agg), signed, dst), dtype=np.uint8)
    data, off = M.engine.pack_messages(msgs)
    data = np.frombuffer(data, dtype=np.uint8)
    nb = (G + 7) // 8
    want = synth.bitmap_of([g not in set(wrong) for g in range(G)])
    bm_new, bm_old = np.zeros(nb, dtype=np.uint8), np.zeros(nb, dtype=np.uint8)
    h = ctypes.c_void_p()
    assert lib.blsbn254_keyset_create(ctx, P8(pks), SZ(n), ctypes.byref(h)) == 0
    if committee:
        members = np.arange(n_com * size, dtype=np.uint32)
        com_off = np.arange(n_com + 1, dtype=np.uint64) * np.uint64(size)
        assert lib.blsbn254_keyset_set_committees(ctx, h, P32(members), P64(com_off), SZ(n_com)) == 0

    def run_new():
        t = time.perf_counter()
        if committee:
            rc = lib.blsbn254_keyset_committee_fast_aggregate_verify_batch_rlc(ctx, h, P32(com), P8(rows), P64(sel_off), P8(data), P64(off), P8(sigs), SZ(G), dst,
                                                                               SZ(len(dst)), NOSEED, P8(bm_new))
        else:
            rc = lib.blsbn254_keyset_fast_aggregate_verify_batch_rlc(ctx, h, P8(rows), P8(data), P64(off), P8(sigs), SZ(G), dst, SZ(len(dst)), NOSEED, P8(bm_new))
        dt = time.perf_counter() - t
        assert rc == 0
        return dt * 1e3

    def run_old():
        t = time.perf_counter()
        if committee:
            rc = lib.blsbn254_keyset_committee_fast_aggregate_verify_batch(ctx, h, P32(com), P8(rows), P64(sel_off), P8(data), P64(off), P8(sigs), SZ(G), dst,
                                                                           SZ(len(dst)), P8(bm_old))
        else:
            rc = lib.blsbn254_keyset_fast_aggregate_verify_batch(ctx, h, P8(rows), P8(data), P64(off), P8(sigs), SZ(G), dst, SZ(len(dst)), P8(bm_old))
        dt = time.perf_counter() - t
        assert rc == 0
        return dt * 1e3

    forms = [("rlc", run_new), ("exact", run_old)]
    for _ in range(WARM):
        for _, fn in forms:
            fn()
    assert bm_new.tobytes() == want and bm_old.tobytes() == want, name
    times = {k: [] for k, _ in forms}
    s0 = rlc_stats()
    for _ in range(REPS):
        for k, fn in forms:
            times[k].append(fn())
    s1 = rlc_stats()
    row = {"registry_keys": n, "committees": n_com, "members_each": size, "groups": G, "message_classes": len(seen), "wrong_signatures": len(wrong),
           "per_call": dict(zip(("decided_groups", "chunks", "failed_chunk_groups", "direct_groups", "classes"), [(b - a) // REPS for a, b in zip(s0, s1)][:5]))}
    for k, _ in forms:
        row[k] = stats(times[k])
    e.profile_enable(True)
    for k, fn in forms:
        e.profile_reset()
        for _ in range(PROF):
            fn()
        row[k]["kernel_ms"] = kernels(PROF)
    e.profile_enable(False); e.profile_reset()
    km = row["rlc"]["kernel_ms"]
    row["weight_kernels_ms"] = round(sum(km.get(x, 0.0) for x in ("ksr_elig", "ksr_weigh_g1", "ksr_weigh_g2")), 4)
    row["chunk_sum_kernels_ms"] = round(sum(km.get(x, 0.0) for x in ("g1_seg_sum", "ksr_chunks", "ksr_gather")), 4)
    row["ratio_to_exact"] = round(row["rlc"]["median_ms"] / row["exact"]["median_ms"], 3)
    row["below_exact"] = below(row["rlc"], row["exact"])
    out["rows"][name] = row
    lib.blsbn254_keyset_destroy(h)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    open(args.out, "w").write(text + "\n")
e.close()
print(json.dumps(out, indent=1))
