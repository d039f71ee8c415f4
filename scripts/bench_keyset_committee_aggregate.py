"""Checked signature aggregation per COMMITTEE of a registered key set (blsbn254_keyset_committee_aggregate_checked_batch) against
what the parent API offers a collector on the same inputs, three steps that are timed and listed one by one:
  (1) the host translation of every (committee, position) to its registry index, with the per-group sort by index that the
      full-width call's canonical order asks for (numpy: one take, one lexsort, the signatures permuted along)
  (2) blsbn254_keyset_aggregate_checked_batch on full-width rows of ceil(n_keys / 8) bytes
  (3) the host compaction of out_sel to the committee rows the committee verify wants (numpy: one gather of bytes, one packbits)
All through the C ABI on numpy buffers.  Per row: warm-up, REPS timed repetitions of each form, alternating; median, quartiles,
min and max of the wall time (host clock around calls that end synchronised).  Registration and set_committees are not part of
the timed call.  Kernel times come from the engine's HIP-event profile in passes of their own, after the wall-time passes.  Both
forms are checked to give the same signatures, statuses and committee rows.  Committee c lists the keys [c size, (c + 1) size)
of the registry in a shuffled order (the uniform row: the registry in order).
Usage: python scripts/bench_keyset_committee_aggregate.py [--out profiles/keyset_committee_aggregate.json] [--reps 20] [--rows 0,1] [--quick] -> JSON"""
import argparse, ctypes, json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import blsbn254_loader; M = blsbn254_loader.load()
from tests import synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join("profiles", "keyset_committee_aggregate.json"))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rows", default="", help="comma-separated row numbers (default: all)")
ap.add_argument("--quick", action="store_true", help="tiny rows: a rehearsal of the script, not a measurement")
args = ap.parse_args()
REPS, WARM, PROF = max(args.reps, 1), 3, 2
# registry keys, committees, members each, groups per committee, a wrong signature in every k-th group or 0, the condition applies, name
ROWS = [(65536, 64, 512, 16, 0, True, "65536 keys, 64 committees of 512, 16 groups each (1024 groups), all honest"),
        (65536, 64, 512, 16, 16, True, "65536 keys, 64 committees of 512, 16 groups each, one wrong signature in every 16th group"),
        (65536, 2048, 32, 16, 0, True, "65536 keys, 2048 committees of 32, 16 groups each (32768 groups), all honest"),
        (65536, 2048, 32, 16, 16, True, "65536 keys, 2048 committees of 32, 16 groups each, one wrong signature in every 16th group"),
        (1024, 1, 1024, 4096, 0, False, "1024 keys, ONE committee of all keys, 4096 groups (uniform)"),
        (1024, 1, 64, 16, 0, False, "1024 keys, one committee of 64, 16 groups (latency)")]
if args.quick:
    ROWS = [(700, 4, 70, 5, 0, True, "quick ragged"), (700, 4, 70, 5, 4, True, "quick ragged, one wrong in every 4th"), (70, 1, 70, 24, 0, False, "quick uniform")]
if args.rows:
    ROWS = [ROWS[int(k)] for k in args.rows.split(",")]
u8, u32, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
P8 = lambda a: a.ctypes.data_as(u8)
P32 = lambda a: a.ctypes.data_as(u32)
P64 = lambda a: a.ctypes.data_as(u64)
SZ = ctypes.c_size_t
dst = M.DEFAULT_DST
e = M.Engine(0)
lib, ctx = e._lib, e._ctx
NMAX = max(r[0] for r in ROWS)
sk_all = np.frombuffer(b"".join(int(synth.sk_of(k)).to_bytes(32, "big") for k in range(NMAX)), dtype=np.uint8).reshape(NMAX, 32)
pk_all = np.frombuffer(e.sk_to_pk_batch(sk_all.tobytes(), NMAX), dtype=np.uint8).reshape(NMAX, 128)
ML = 32                                                                # message length (synth.msg_of)


def stats(ms):
    a = np.sort(np.array(ms))
    q1, med, q3 = (float(np.percentile(a, p)) for p in (25, 50, 75))
    return {"median_ms": round(med, 3), "spread_ms": round(q3 - q1, 3), "q1_ms": round(q1, 3), "q3_ms": round(q3, 3), "min_ms": round(float(a[0]), 3),
            "max_ms": round(float(a[-1]), 3), "reps": len(ms)}


def kernels(reps):
    pr = e.profile_read()
    return {n: round(v["total_ms"] / reps, 4) for n, v in sorted(pr.items()) if v["total_ms"] / reps > 0.002}


out = {"method": "wall: host clock around C-ABI calls that end synchronised, %d warm-up + %d timed repetitions per form, alternating; spread = interquartile "
                 "range; kernel_ms: HIP-event profile, mean of %d further repetitions in passes of their own" % (WARM, REPS, PROF), "rows": {}}
rnd = np.random.RandomState(15)
for n, n_com, size, per, wrong_every, conditioned, name in ROWS:
    G = n_com * per
    pks = np.ascontiguousarray(pk_all[:n])
    uniform = n_com == 1 and size == n
    mem2 = np.arange(n_com * size, dtype=np.uint32).reshape(n_com, size)
    if not uniform:
        mem2 = np.stack([rnd.permutation(r) for r in mem2]).astype(np.uint32)
    members = np.ascontiguousarray(mem2.reshape(-1))
    com_off = np.arange(n_com + 1, dtype=np.uint64) * np.uint64(size)
    com = np.repeat(np.arange(n_com, dtype=np.uint32), per)
    bits = rnd.random_sample((G, size)) < 2 / 3
    bits[:, 0] = True; bits[:, 1 % size] = True
    grp, pos = np.nonzero(bits)                                         # entries in group order, positions increasing inside a group
    pos = pos.astype(np.uint32)
    N = len(pos)
    soff = np.zeros(G + 1, dtype=np.uint64)
    soff[1:] = np.cumsum(np.bincount(grp, minlength=G))
    crb, rb = (size + 7) // 8, (n + 7) // 8
    sel_off = np.arange(G + 1, dtype=np.uint64) * np.uint64(crb)
    msg_tab = np.frombuffer(b"".join(synth.msg_of(80000 + g) for g in range(G)), dtype=np.uint8).reshape(G, ML)
    moff = np.arange(G + 1, dtype=np.uint64) * ML
    # every entry signed by its member's key on its group's message; the wrong ones by another key of the registry
    signer = mem2[com[grp], pos].astype(np.int64)
    bad_entries = np.array([int(soff[g]) + 1 for g in range(0, G, wrong_every)] if wrong_every else [], dtype=np.int64)
    signer[bad_entries] = (signer[bad_entries] + 1) % n
    sigs = np.zeros(64 * N, dtype=np.uint8)
    STEP = 1 << 19
    for lo in range(0, N, STEP):                                        # (by pieces: the per-entry messages are built on the host)
        hi = min(N, lo + STEP)
        sk = np.ascontiguousarray(sk_all[signer[lo:hi]]); em = np.ascontiguousarray(msg_tab[grp[lo:hi]])
        emoff = np.arange(hi - lo + 1, dtype=np.uint64) * ML
        assert lib.blsbn254_sign_batch(ctx, P8(sk), P8(em), P64(emoff), SZ(hi - lo), dst, SZ(len(dst)), P8(sigs[64 * lo:])) == 0
    want_bits = bits.copy()
    want_bits[grp[bad_entries], pos[bad_entries]] = False
    want_rows = np.packbits(want_bits, axis=1, bitorder="little")
    h = ctypes.c_void_p()
    assert lib.blsbn254_keyset_create(ctx, P8(pks), SZ(n), ctypes.byref(h)) == 0
    assert lib.blsbn254_keyset_set_committees(ctx, h, P32(members), P64(com_off), SZ(n_com)) == 0
    o_new, r_new, s_new = np.zeros(64 * G, dtype=np.uint8), np.zeros(crb * G, dtype=np.uint8), np.full(G, 0xff, dtype=np.uint8)
    o_old, wide, s_old = np.zeros(64 * G, dtype=np.uint8), np.zeros(rb * G, dtype=np.uint8), np.full(G, 0xff, dtype=np.uint8)
    r_old = np.zeros((G, crb), dtype=np.uint8)
    garange = np.arange(G)[:, None]

    def run_new():
        t = time.perf_counter()
        rc = lib.blsbn254_keyset_committee_aggregate_checked_batch(ctx, h, P32(com), P32(pos), P8(sigs), P64(soff), P8(msg_tab), P64(moff), P64(sel_off), SZ(G), dst,
                                                                   SZ(len(dst)), P8(o_new), P8(r_new), P8(s_new))
        dt = time.perf_counter() - t
        assert rc == 0
        return dt * 1e3, 0.0, 0.0, 0.0

    def run_old():
        t = time.perf_counter()
        idx = members[com_off[com[grp]].astype(np.int64) + pos]         # (1) positions to registry indices, sorted inside every group
        order = np.lexsort((idx, grp))
        idx_s = np.ascontiguousarray(idx[order]); sig_s = np.ascontiguousarray(sigs.reshape(N, 64)[order])
        t1 = time.perf_counter()
        rc = lib.blsbn254_keyset_aggregate_checked_batch(ctx, h, P32(idx_s), P8(sig_s), P64(soff), P8(msg_tab), P64(moff), SZ(G), dst, SZ(len(dst)), P8(o_old),
                                                         P8(wide), P8(s_old))      # (2)
        assert rc == 0
        t2 = time.perf_counter()
        key = mem2[com]                                                 # (3) the committee rows: bit j = bit members[j] of the full-width row
        byte = wide.reshape(G, rb)[garange, key >> 3]
        r_old[:] = np.packbits((byte >> (key & 7).astype(np.uint8)) & 1, axis=1, bitorder="little")
        t3 = time.perf_counter()
        return (t3 - t) * 1e3, (t1 - t) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3

    for _ in range(WARM):
        run_new(); run_old()
    assert s_new.tobytes() == bytes(G) == s_old.tobytes() and o_new.tobytes() == o_old.tobytes(), name
    assert r_new.tobytes() == want_rows.tobytes() == r_old.tobytes(), name
    ag0, fw0 = (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 4)()
    lib.blsbn254_keyset_committee_aggregate_stats(ctx, ag0); lib.blsbn254_keyset_aggregate_stats(ctx, fw0)
    t_new, t_old, t_parts = [], [], []
    for _ in range(REPS):
        t_new.append(run_new()[0])
        o = run_old(); t_old.append(o[0]); t_parts.append(o[1:])
    ag1, fw1 = (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 4)()
    lib.blsbn254_keyset_committee_aggregate_stats(ctx, ag1); lib.blsbn254_keyset_aggregate_stats(ctx, fw1)
    assert [ag1[i] - ag0[i] for i in range(4)] == [fw1[i] - fw0[i] for i in range(4)], name
    parts = np.median(np.array(t_parts), axis=0)
    row = {"registry_keys": n, "committees": n_com, "members_each": size, "groups": G, "entries": int(N), "wrong_signatures": int(len(bad_entries)),
           "fallback_groups_per_call": int((ag1[1] - ag0[1]) // REPS), "committee": stats(t_new), "full_width_three_steps": stats(t_old),
           "full_width_median_ms": {"translate_and_sort": round(float(parts[0]), 3), "keyset_aggregate_checked_batch": round(float(parts[1]), 3),
                                    "compact_rows": round(float(parts[2]), 3)},
           "out_sel_bytes": {"committee": int(crb * G), "full_width": int(rb * G)}}
    e.profile_enable(True)
    for key, fn in (("committee", run_new), ("full_width_three_steps", run_old)):
        e.profile_reset()
        for _ in range(PROF):
            fn()
        row[key]["kernel_ms"] = kernels(PROF)
    e.profile_enable(False); e.profile_reset()
    a, b = row["committee"], row["full_width_three_steps"]
    row["condition_applies"] = conditioned
    row["below_by_more_than_both_spreads"] = bool(a["median_ms"] + a["spread_ms"] + b["spread_ms"] < b["median_ms"])
    row["below_the_full_width_call_alone"] = bool(a["median_ms"] < float(parts[1]))
    out["rows"][name] = row
    lib.blsbn254_keyset_destroy(h)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    open(args.out, "w").write(json.dumps(out, indent=1) + "\n")          # after every row: a run that is cut short keeps what it measured
    print(name, json.dumps(row), flush=True)
e.close()
print("done")
