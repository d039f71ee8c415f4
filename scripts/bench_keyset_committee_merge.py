"""Checked merge of partial aggregates per COMMITTEE of a registered key set (blsbn254_keyset_committee_merge_checked_batch) against
what the parent API offers an intermediate node on the same inputs, three steps that are timed and listed one by one:
  (1) the host scatter of every committee-wide contribution row to a row of ceil(n_keys / 8) bytes (numpy: the set bits of the
      rows, one take through the member lists, one bitwise_or.at into zeroed rows)
  (2) blsbn254_keyset_merge_checked_batch on the full-width rows, in as few calls as its limit of 2^30 bytes of rows allows
  (3) the host compaction of out_sel to the committee rows the committee verify wants (numpy: one gather of bytes, one packbits)
Where the one committee is the registry in order (the uniform row) the rows are the same bytes and the parent's form is its call
alone.  All through the C ABI on numpy buffers.  Per row: warm-up, REPS timed repetitions of each form, alternating; median,
quartiles, min and max of the wall time (host clock around calls that end synchronised); a row whose parent form takes more
than a second per repetition gets fewer of them, and says so.  Registration and set_committees are not part of the timed call.
Kernel times come from the engine's HIP-event profile in passes of their own, after the wall-time passes.  Both forms are
checked to give the same signatures, statuses, used bits and committee rows before anything is timed.  Committee c lists the keys
[c size, (c + 1) size) of the registry in a shuffled order; contribution k of a group names the positions [k K, (k + 1) K) of its
committee and is signed by the sum of those members' secrets, a wrong one by that sum + 1.
Usage: python scripts/bench_keyset_committee_merge.py [--out profiles/keyset_committee_merge.json] [--reps 20] [--rows 0,1] [--quick] -> JSON"""
import argparse, ctypes, json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import blsbn254_loader; M = blsbn254_loader.load()
from tests import synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join("profiles", "keyset_committee_merge.json"))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rows", default="", help="comma-separated row numbers (default: all)")
ap.add_argument("--quick", action="store_true", help="tiny rows: a rehearsal of the script, not a measurement")
args = ap.parse_args()
C = 16                                                                 # contributions per group
MAX_ROW_BYTES = 1 << 30                                                # of one blsbn254_keyset_merge_checked_batch
# registry keys, committees, members each, groups per committee, positions per contribution, a wrong contribution in every k-th group or 0, name
SHAPES = [(65536, 64, 512, 16, 32, "65536 keys, 64 committees of 512, 16 groups each (1024 groups)"),
          (65536, 2048, 32, 16, 2, "65536 keys, 2048 committees of 32, 16 groups each (32768 groups)"),
          (1024, 1, 1024, 4096, 42, "1024 keys, ONE committee of all keys, 4096 groups (uniform)"),
          (1024, 1, 64, 16, 4, "1024 keys, one committee of 64, 16 groups (latency)")]
if args.quick:
    SHAPES = [(700, 4, 70, 5, 4, "quick ragged"), (70, 1, 70, 24, 4, "quick uniform")]
ROWS = [s[:5] + (w, s[5] + (", one wrong contribution in every 16th group" if w else ", all honest")) for s in SHAPES for w in (0, 16)]
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
R = synth.R
NMAX = max(r[0] for r in ROWS)
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
    return {n: round(v["total_ms"] / reps, 4) for n, v in sorted(pr.items()) if v["total_ms"] / reps > 0.002}


out = {"method": "wall: host clock around C-ABI calls that end synchronised, warm-up + timed repetitions per form, alternating (3 + --reps, or 1 + 5 where the "
                 "parent form takes more than a second); spread = interquartile range; kernel_ms: HIP-event profile, mean of further repetitions in passes of "
                 "their own", "rows": {}}
rnd = np.random.RandomState(16)
for n, n_com, size, per, K, wrong_every, name in ROWS:
    G = n_com * per
    N = G * C
    assert C * K <= size
    pks = np.ascontiguousarray(pk_all[:n])
    uniform = n_com == 1 and size == n
    mem2 = np.arange(n_com * size, dtype=np.uint32).reshape(n_com, size)
    if not uniform:
        mem2 = np.stack([rnd.permutation(r) for r in mem2]).astype(np.uint32)
    members = np.ascontiguousarray(mem2.reshape(-1))
    com_off = np.arange(n_com + 1, dtype=np.uint64) * np.uint64(size)
    com = np.repeat(np.arange(n_com, dtype=np.uint32), per)
    crb, rb = (size + 7) // 8, (n + 7) // 8
    cbits = np.zeros((C, size), dtype=bool)
    for k in range(C):
        cbits[k, k * K:(k + 1) * K] = True
    crows = np.packbits(cbits, axis=1, bitorder="little")               # (C, crb)
    rows = np.ascontiguousarray(np.tile(crows, (G, 1)))                 # (N, crb): the call's contribution rows
    coff = np.arange(G + 1, dtype=np.uint64) * np.uint64(C)
    roff = np.arange(G + 1, dtype=np.uint64) * np.uint64(C * crb)
    sel_off = np.arange(G + 1, dtype=np.uint64) * np.uint64(crb)
    msg_tab = np.frombuffer(b"".join(synth.msg_of(80000 + g) for g in range(G)), dtype=np.uint8).reshape(G, ML)
    moff = np.arange(G + 1, dtype=np.uint64) * ML
    # the secret of contribution k of committee c, and that + 1 behind them
    csk = [sum(sk_int[i] for i in mem2[c, k * K:(k + 1) * K]) % R for c in range(n_com) for k in range(C)]
    sk_tab = np.frombuffer(b"".join((s or 1).to_bytes(32, "big") for s in csk + [(s + 1) % R or 1 for s in csk]), dtype=np.uint8).reshape(2 * n_com * C, 32)
    grp = np.repeat(np.arange(G), C)
    signer = (com[grp].astype(np.int64) * C + np.tile(np.arange(C), G))
    bad = np.array([g * C + 1 for g in range(0, G, wrong_every)] if wrong_every else [], dtype=np.int64)
    signer[bad] += n_com * C
    sigs = np.zeros(64 * N, dtype=np.uint8)
    STEP = 1 << 19
    for lo in range(0, N, STEP):                                        # (by pieces: the per-contribution messages are built on the host)
        hi = min(N, lo + STEP)
        sk = np.ascontiguousarray(sk_tab[signer[lo:hi]]); em = np.ascontiguousarray(msg_tab[grp[lo:hi]])
        emoff = np.arange(hi - lo + 1, dtype=np.uint64) * ML
        assert lib.blsbn254_sign_batch(ctx, P8(sk), P8(em), P64(emoff), SZ(hi - lo), dst, SZ(len(dst)), P8(sigs[64 * lo:])) == 0
    want_used = np.ones(N, dtype=bool); want_used[bad] = False
    want_rows = np.zeros((G, crb), dtype=np.uint8)
    for k in range(C):
        want_rows |= crows[k][None, :] * want_used.reshape(G, C)[:, k][:, None].astype(np.uint8)
    h = ctypes.c_void_p()
    assert lib.blsbn254_keyset_create(ctx, P8(pks), SZ(n), ctypes.byref(h)) == 0
    assert lib.blsbn254_keyset_set_committees(ctx, h, P32(members), P64(com_off), SZ(n_com)) == 0
    o_new, r_new, s_new = np.zeros(64 * G, dtype=np.uint8), np.zeros(crb * G, dtype=np.uint8), np.full(G, 0xff, dtype=np.uint8)
    u_new = np.zeros((N + 7) // 8, dtype=np.uint8)
    o_old, wide_out, s_old = np.zeros(64 * G, dtype=np.uint8), np.zeros(rb * G, dtype=np.uint8), np.full(G, 0xff, dtype=np.uint8)
    u_old = np.zeros((N + 7) // 8, dtype=np.uint8)
    r_old = np.zeros((G, crb), dtype=np.uint8)
    garange = np.arange(G)[:, None]
    g_call = max(1, min(G, (MAX_ROW_BYTES // rb) // C))                 # groups per parent call (C = 16: whole bytes of `used`)
    calls = [(lo, min(G, lo + g_call)) for lo in range(0, G, g_call)]
    rows3 = rows.reshape(G, C * crb)

    def run_new():
        t = time.perf_counter()
        rc = lib.blsbn254_keyset_committee_merge_checked_batch(ctx, h, P32(com), P8(rows), P64(roff), P8(sigs), P64(coff), P8(msg_tab), P64(moff), P64(sel_off), SZ(G),
                                                               dst, SZ(len(dst)), P8(o_new), P8(r_new), P8(u_new), P8(s_new))
        dt = time.perf_counter() - t
        assert rc == 0
        return dt * 1e3, 0.0, 0.0, 0.0

    def run_old():
        t_scatter = t_call = 0.0
        for lo, hi in calls:
            t = time.perf_counter()
            if uniform:
                wide = rows3[lo:hi]                                     # the committee is the registry in order: the same bytes
            else:                                                       # (1) every set bit j of a row to bit members[j] of a zeroed full-width row
                bits = np.unpackbits(rows3[lo:hi].reshape((hi - lo) * C, crb), axis=1, count=size, bitorder="little")
                s_idx, p = np.nonzero(bits)
                key = mem2[com[lo:hi][s_idx // C], p].astype(np.int64)
                wide = np.zeros((hi - lo) * C * rb, dtype=np.uint8)
                np.bitwise_or.at(wide, s_idx * rb + (key >> 3), (1 << (key & 7)).astype(np.uint8))
            t1 = time.perf_counter()
            off = coff[lo:hi + 1]                                       # (the call indexes rows and signatures by the offsets as given)
            base = int(off[0])
            rc = lib.blsbn254_keyset_merge_checked_batch(ctx, h, ctypes.cast(ctypes.c_void_p(wide.ctypes.data - base * rb), u8), P8(sigs), P64(off), P8(msg_tab), P64(moff[lo:]),
                                                         SZ(hi - lo), dst, SZ(len(dst)), P8(o_old[64 * lo:]), P8(wide_out[rb * lo:]), P8(u_old[base // 8:]),
                                                         P8(s_old[lo:]))      # (2)
            assert rc == 0
            t2 = time.perf_counter()
            t_scatter += t1 - t; t_call += t2 - t1
        t = time.perf_counter()
        if uniform:
            r_old[:] = wide_out.reshape(G, rb)
        else:
            key = mem2[com]                                             # (3) the committee rows: bit j = bit members[j] of the full-width row
            byte = wide_out.reshape(G, rb)[garange, key >> 3]
            r_old[:] = np.packbits((byte >> (key & 7).astype(np.uint8)) & 1, axis=1, bitorder="little")
        t_compact = time.perf_counter() - t
        return (t_scatter + t_call + t_compact) * 1e3, t_scatter * 1e3, t_call * 1e3, t_compact * 1e3

    run_new()
    first = run_old()[0]
    slow = first > 1000.0
    warm, reps, prof = (0, min(args.reps, 5), 1) if slow else (2, max(args.reps, 1), 2)
    for _ in range(warm):
        run_new(); run_old()
    assert s_new.tobytes() == bytes(G) == s_old.tobytes() and o_new.tobytes() == o_old.tobytes(), name
    assert r_new.tobytes() == want_rows.tobytes() == r_old.tobytes(), name
    assert np.array_equal(np.unpackbits(u_new, count=N, bitorder="little").astype(bool), want_used) and u_new.tobytes() == u_old.tobytes(), name
    cm0, fw0 = (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 4)()
    lib.blsbn254_keyset_committee_merge_stats(ctx, cm0); lib.blsbn254_keyset_merge_stats(ctx, fw0)
    t_new, t_old, t_parts = [], [], []
    for _ in range(reps):
        t_new.append(run_new()[0])
        o = run_old(); t_old.append(o[0]); t_parts.append(o[1:])
    cm1, fw1 = (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 4)()
    lib.blsbn254_keyset_committee_merge_stats(ctx, cm1); lib.blsbn254_keyset_merge_stats(ctx, fw1)
    assert [cm1[i] - cm0[i] for i in range(4)] == [fw1[i] - fw0[i] for i in range(4)], name
    parts = np.median(np.array(t_parts), axis=0)
    row = {"registry_keys": n, "committees": n_com, "members_each": size, "groups": G, "contributions": int(N), "positions_per_contribution": K,
           "wrong_contributions": int(len(bad)), "fallback_groups_per_call": int((cm1[1] - cm0[1]) // reps), "warm_up": warm + 1,
           "committee": stats(t_new), "parent_form": stats(t_old), "parent_calls": len(calls),
           "parent_form_median_ms": {"scatter_rows": round(float(parts[0]), 3), "keyset_merge_checked_batch": round(float(parts[1]), 3),
                                     "compact_rows": round(float(parts[2]), 3)},
           "row_bytes_in": {"committee": int(crb * N), "full_width": int(rb * N)}, "out_sel_bytes": {"committee": int(crb * G), "full_width": int(rb * G)}}
    e.profile_enable(True)
    for key, fn in (("committee", run_new), ("parent_form", run_old)):
        e.profile_reset()
        for _ in range(prof):
            fn()
        row[key]["kernel_ms"] = kernels(prof)
    e.profile_enable(False); e.profile_reset()
    a, b = row["committee"], row["parent_form"]
    ksum = sum(a["kernel_ms"].values())
    row["kcm_select_share_of_kernel_time"] = round(a["kernel_ms"].get("kcm_select", 0.0) / ksum, 4) if ksum else None
    row["committee_faster_than_parent_form"] = bool(a["median_ms"] < b["median_ms"])
    row["difference_beyond_both_spreads"] = bool(abs(a["median_ms"] - b["median_ms"]) > a["spread_ms"] + b["spread_ms"])
    out["rows"][name] = row
    lib.blsbn254_keyset_destroy(h)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    open(args.out, "w").write(json.dumps(out, indent=1) + "\n")          # after every row: a run that is cut short keeps what it measured
    print(name, json.dumps(row), flush=True)
e.close()
print("done")
