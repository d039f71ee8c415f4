"""FastAggregateVerify over the COMMITTEES of a registered key set (blsbn254_keyset_committee_fast_aggregate_verify_batch) against
what the parent API offers on the same inputs:
  (a) blsbn254_keyset_fast_aggregate_verify_batch on full-width rows, the host's scatter of the committee rows over the registry
      (numpy, packed bytes) counted, because a caller has to do it; the call alone is reported beside it
  (b) where the committees are disjoint: one key set per committee and one call each, registration outside the timed region
All through the C ABI on numpy buffers.  Per row: warm-up, REPS timed repetitions of each form, alternating; median, quartiles,
min and max of the wall time (host clock around calls that end synchronised).  Kernel times come from the engine's HIP-event
profile in passes of their own.  Committee c lists the keys [c size, (c + 1) size) of the registry and the groups come committee
by committee, so the committee rows ARE the rows of form (b); every form is checked to give the same bitmap.
Usage: python scripts/bench_keyset_committee.py [--out profiles/keyset_committee.json] [--reps 20] [--only 0,2] [--quick] -> JSON
(--only: row numbers; the rows of an existing --out file are kept)"""
import argparse, ctypes, json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import blsbn254_loader; M = blsbn254_loader.load()
from tests import synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join("profiles", "keyset_committee.json"))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--only", default="")
ap.add_argument("--quick", action="store_true", help="tiny rows: a rehearsal of the script, not a measurement")
args = ap.parse_args()
REPS, WARM, PROF = max(args.reps, 1), 3, 3
# registry keys, committees, members each, groups per committee, form (b) measured, name
ROWS = [(65536, 64, 512, 16, True, "65536 keys, 64 committees of 512, 16 groups each (1024 groups)"),
        (65536, 2048, 32, 16, True, "65536 keys, 2048 committees of 32, 16 groups each (32768 groups, M = 65536)"),
        (1024, 1, 1024, 4096, False, "1024 keys, ONE committee of all keys, 4096 groups (uniform)"),
        (1024, 1, 64, 16, True, "1024 keys, one committee of 64, 16 groups (latency floor)")]
if args.quick:
    ROWS = [(700, 4, 70, 5, True, "quick ragged"), (70, 1, 70, 24, False, "quick uniform")]
only = [int(t) for t in args.only.split(",") if t] or list(range(len(ROWS)))
u8, u32, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
P8 = lambda a: a.ctypes.data_as(u8)
P32 = lambda a: a.ctypes.data_as(u32)
P64 = lambda a: a.ctypes.data_as(u64)
SZ = ctypes.c_size_t
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


out = {"method": "wall: host clock around C-ABI calls that end synchronised, %d warm-up + %d timed repetitions per form, alternating; spread = interquartile "
                 "range; kernel_ms: HIP-event profile, mean of %d further repetitions in passes of their own" % (WARM, REPS, PROF), "rows": {}}
if args.only and os.path.exists(args.out):
    out["rows"] = json.load(open(args.out)).get("rows", {})
rnd = np.random.RandomState(12)
for ri in only:
    n, n_com, size, per, with_b, name = ROWS[ri]
    G = n_com * per
    pks = np.ascontiguousarray(pk_all[:n])
    members = np.arange(n_com * size, dtype=np.uint32)                  # committee c = keys [c size, (c + 1) size)
    com_off = (np.arange(n_com + 1, dtype=np.uint64) * np.uint64(size))
    com = np.repeat(np.arange(n_com, dtype=np.uint32), per)
    bits = rnd.random_sample((G, size)) < 2 / 3
    bits[:, 0] = True
    rows = np.packbits(bits, axis=1, bitorder="little")                 # G rows of ceil(size / 8) bytes, LSB-first
    crb = rows.shape[1]
    sel_off = np.arange(G + 1, dtype=np.uint64) * np.uint64(crb)
    sk_mat = sks[:n_com * size].reshape(n_com, size)
    agg = [int(sum(sk_mat[g // per][bits[g]])) % R or 1 for g in range(G)]
    msgs = [synth.msg_of(60000 + g) for g in range(G)]
    sigs = np.frombuffer(e.sign_batch(b"".join(s.to_bytes(32, "big") for s in agg), msgs, dst), dtype=np.uint8)
    for g in range(6, G, 7):
        msgs[g] = bytes([msgs[g][0] ^ 1]) + msgs[g][1:]
    data, off = M.engine.pack_messages(msgs)
    data = np.frombuffer(data, dtype=np.uint8)
    nb = (G + 7) // 8
    want = synth.bitmap_of([g % 7 != 6 for g in range(G)])
    bm_new, bm_a, bm_b = np.zeros(nb, dtype=np.uint8), np.zeros(nb, dtype=np.uint8), np.zeros(nb, dtype=np.uint8)
    h = ctypes.c_void_p()
    assert lib.blsbn254_keyset_create(ctx, P8(pks), SZ(n), ctypes.byref(h)) == 0
    st0 = (ctypes.c_uint64 * 4)()
    lib.blsbn254_keyset_committee_stats(ctx, st0)
    t_set = []
    for _ in range(WARM + min(REPS, 5)):
        t = time.perf_counter()
        assert lib.blsbn254_keyset_set_committees(ctx, h, P32(members), P64(com_off), SZ(n_com)) == 0
        t_set.append((time.perf_counter() - t) * 1e3)

    def run_new():
        t = time.perf_counter()
        rc = lib.blsbn254_keyset_committee_fast_aggregate_verify_batch(ctx, h, P32(com), P8(rows), P64(sel_off), P8(data), P64(off), P8(sigs), SZ(G), dst,
                                                                       SZ(len(dst)), P8(bm_new))
        dt = time.perf_counter() - t
        assert rc == 0
        return dt * 1e3, 0.0

    rb = (n + 7) // 8
    jj = np.nonzero(bits)                                               # (group, member position) of every set bit: the caller's knowledge
    uniform = n_com == 1 and size == n

    def run_a():
        t = time.perf_counter()
        if uniform:
            wide = rows                                                 # the committee is the registry: identical rows, nothing to scatter
        else:
            key = members[com_off[com[jj[0]]].astype(np.int64) + jj[1]]
            wide = np.zeros(G * rb, dtype=np.uint8)
            np.bitwise_or.at(wide, jj[0] * rb + (key >> 3), (1 << (key & 7)).astype(np.uint8))
        ts = time.perf_counter()
        rc = lib.blsbn254_keyset_fast_aggregate_verify_batch(ctx, h, P8(wide), P8(data), P64(off), P8(sigs), SZ(G), dst, SZ(len(dst)), P8(bm_a))
        dt = time.perf_counter() - t
        assert rc == 0
        return dt * 1e3, (ts - t) * 1e3

    # form (b): one key set per committee, its groups' rows, messages and signatures as one call each (prepared outside the timed region)
    subs = []
    if with_b:
        for c in range(n_com):
            hc = ctypes.c_void_p()
            assert lib.blsbn254_keyset_create(ctx, P8(np.ascontiguousarray(pk_all[c * size:(c + 1) * size])), SZ(size), ctypes.byref(hc)) == 0
            d, o = M.engine.pack_messages(msgs[c * per:(c + 1) * per])
            subs.append((hc, np.ascontiguousarray(rows[c * per:(c + 1) * per]), np.frombuffer(d, dtype=np.uint8), o,
                         np.ascontiguousarray(sigs[64 * c * per:64 * (c + 1) * per]), np.zeros((per + 7) // 8, dtype=np.uint8)))
    bits_b = np.zeros(G, dtype=bool)

    def run_b():
        t = time.perf_counter()
        for c, (hc, r, d, o, s, bm) in enumerate(subs):
            rc = lib.blsbn254_keyset_fast_aggregate_verify_batch(ctx, hc, P8(r), P8(d), P64(o), P8(s), SZ(per), dst, SZ(len(dst)), P8(bm))
            assert rc == 0
            bits_b[c * per:(c + 1) * per] = np.unpackbits(bm, count=per, bitorder="little")
        bm_b[:] = np.packbits(bits_b, bitorder="little")
        return (time.perf_counter() - t) * 1e3, 0.0

    forms = [("committee", run_new), ("full_width_with_scatter", run_a)] + ([("key_set_per_committee", run_b)] if with_b else [])
    for _ in range(WARM):
        for _, fn in forms:
            fn()
    assert bm_new.tobytes() == want and bm_a.tobytes() == want and (not with_b or bm_b.tobytes() == want), name
    times = {k: [] for k, _ in forms}
    scat = []
    for _ in range(REPS):
        for k, fn in forms:
            r = fn()
            times[k].append(r[0])
            if k == "full_width_with_scatter":
                scat.append(r[1])
    row = {"registry_keys": n, "committees": n_com, "members_each": size, "groups": G, "selected_keys": int(bits.sum()), "set_committees": stats(t_set[WARM:])}
    for k, _ in forms:
        row[k] = stats(times[k])
    row["full_width_call_alone"] = stats(list(np.array(times["full_width_with_scatter"]) - np.array(scat)))
    row["host_scatter_median_ms"] = round(float(np.median(scat)), 3)
    e.profile_enable(True)
    for k, fn in forms:
        e.profile_reset()
        for _ in range(PROF):
            fn()
        row[k]["kernel_ms"] = kernels(PROF)
    e.profile_enable(False); e.profile_reset()
    km = row["committee"]["kernel_ms"]
    row["committee_sum_kernels_ms"] = round(sum(km.get(x, 0.0) for x in ("kc_count", "kc_word_sum", "g2_seg_sum", "kc_finish")), 4)
    ka = row["full_width_with_scatter"]["kernel_ms"]
    row["full_width_sum_kernels_ms"] = round(sum(ka.get(x, 0.0) for x in ("ks_count", "ks_word_sum", "ks_group_sum")), 4)
    row["ratio_to_full_width_call_alone"] = round(row["committee"]["median_ms"] / row["full_width_call_alone"]["median_ms"], 3)
    row["below_full_width_with_scatter"] = below(row["committee"], row["full_width_with_scatter"])
    row["below_full_width_call_alone"] = below(row["committee"], row["full_width_call_alone"])
    if with_b:
        row["below_key_set_per_committee"] = below(row["committee"], row["key_set_per_committee"])
    st = (ctypes.c_uint64 * 4)()
    lib.blsbn254_keyset_committee_stats(ctx, st)
    row["complement_share_of_committee_groups"] = round((st[1] - st0[1]) / max(st[0] - st0[0], 1), 3)
    out["rows"][name] = row
    for s in subs:
        lib.blsbn254_keyset_destroy(s[0])
    lib.blsbn254_keyset_destroy(h)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    open(args.out, "w").write(text + "\n")
e.close()
print(json.dumps(out, indent=1))
