"""The wire-format forms of the checked aggregation and merge calls (blsbn254_keyset_*_checked_batch_compressed) against what a
caller that holds 32-byte signatures had to do before them, on the same inputs, all through the C ABI on numpy buffers:
  a  the uncompressed call on uncompressed input (the price of the wire format is c / a)
  b  the parent's way for wire bytes: blsbn254_g1_inflate_batch -> the uncompressed call -> blsbn254_g1_compress_batch of out_sigs
  c  the compressed call
Per row: warm-up, REPS timed repetitions of each form, alternating; median, quartiles, min and max of the wall time (host clock
around calls that end synchronised).  Registration is not part of the timed call.  Kernel times come from the engine's HIP-event
profile in passes of their own, after the wall-time passes: PROF passes of one repetition each, so that the scan kernels have a
median and a spread of their own -- the fused scan (ka_scan_wire in c) against the staged form (g1_inflate in b + ka_scan in a).
Every form must return the expected statuses and rows, and c the bytes of b.
Usage: python scripts/bench_keyset_wire.py [--out profiles/keyset_wire.json] [--reps 20] [--rows 0,1,..] [--quick] -> JSON"""
import argparse, ctypes, json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import blsbn254_loader; M = blsbn254_loader.load()
from tests import synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join("profiles", "keyset_wire.json"))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rows", default="", help="comma-separated row numbers (default: all)")
ap.add_argument("--quick", action="store_true", help="tiny rows: a rehearsal of the script, not a measurement")
args = ap.parse_args()
REPS, WARM, PROF = max(args.reps, 1), 3, 5
# kind, the condition against b applies, name, then per kind:
#   collector: groups, keys, participation, a wrong signature in every k-th group or 0
#   committee: registry keys, committees, members each, groups per committee
#   merge:     groups, keys, contributions per group, keys per contribution
ROWS = [("collector", True, "collector: 4096 groups, 1024 keys, 2/3 participation, all honest", 4096, 1024, 2 / 3, 0),
        ("collector", True, "collector: 4096 groups, 1024 keys, 2/3 participation, one wrong signature in every 16th group", 4096, 1024, 2 / 3, 16),
        ("collector", True, "collector: 4096 groups, 64 keys, all signing", 4096, 64, 1.0, 0),
        ("committee", False, "committee collector: 65536 keys, 64 committees of 512, 16 groups each (1024 groups)", 65536, 64, 512, 16),
        ("merge", False, "merge: 4096 groups, 1024 keys, 16 contributions of 42 keys", 4096, 1024, 16, 42),
        ("collector", False, "collector: 16 groups, 64 keys, all signing (for the record)", 16, 64, 1.0, 0)]
if args.quick:
    ROWS = [("collector", True, "quick collector", 24, 70, 2 / 3, 0), ("collector", True, "quick collector, one wrong in every 4th", 24, 70, 2 / 3, 4),
            ("committee", False, "quick committee collector", 700, 4, 70, 5), ("merge", False, "quick merge", 24, 70, 4, 9)]
if args.rows:
    ROWS = [ROWS[int(k)] for k in args.rows.split(",")]
u8, u32, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
P8 = lambda a: a.ctypes.data_as(u8)
P32 = lambda a: a.ctypes.data_as(u32)
P64 = lambda a: a.ctypes.data_as(u64)
SZ = ctypes.c_size_t
dst = M.DEFAULT_DST
DL = SZ(len(dst))
e = M.Engine(0)
lib, ctx = e._lib, e._ctx
R = synth.R
NMAX = max(r[4] if r[0] != "committee" else r[3] for r in ROWS)
sk_int = [int(synth.sk_of(k)) for k in range(NMAX + 1)]
sk_all = np.frombuffer(b"".join(s.to_bytes(32, "big") for s in sk_int), dtype=np.uint8).reshape(NMAX + 1, 32)
pk_all = np.frombuffer(e.sk_to_pk_batch(sk_all[:NMAX].tobytes(), NMAX), dtype=np.uint8).reshape(NMAX, 128)
ML = 32                                                                # message length (synth.msg_of)
STEP = 1 << 19


def stats(ms):
    a = np.sort(np.array(ms))
    q1, med, q3 = (float(np.percentile(a, p)) for p in (25, 50, 75))
    return {"median_ms": round(med, 3), "spread_ms": round(q3 - q1, 3), "q1_ms": round(q1, 3), "q3_ms": round(q3, 3), "min_ms": round(float(a[0]), 3),
            "max_ms": round(float(a[-1]), 3), "reps": len(ms)}


def sign(sk_rows, msg_rows):
    """one signature per row of secret keys on the message of the same row, by pieces (the per-entry messages are host arrays)"""
    n = len(sk_rows)
    sigs = np.zeros(64 * max(n, 1), dtype=np.uint8)
    for lo in range(0, n, STEP):
        hi = min(n, lo + STEP)
        sk = np.ascontiguousarray(sk_rows[lo:hi]); em = np.ascontiguousarray(msg_rows[lo:hi])
        emoff = np.arange(hi - lo + 1, dtype=np.uint64) * ML
        assert lib.blsbn254_sign_batch(ctx, P8(sk), P8(em), P64(emoff), SZ(hi - lo), dst, DL, P8(sigs[64 * lo:])) == 0
    return sigs


def kernel_passes(fn):
    """PROF profiled passes of one repetition each: {kernel: [ms per pass]}"""
    per = {}
    for _ in range(PROF):
        e.profile_reset()
        fn()
        for n, v in e.profile_read().items():
            per.setdefault(n, []).append(v["total_ms"])
    return per


out = {"method": "wall: host clock around C-ABI calls that end synchronised, %d warm-up + %d timed repetitions per form, the forms alternating; spread = "
                 "interquartile range; kernel_ms: HIP-event profile, median of %d further passes of one repetition each, in passes of their own; a = the "
                 "uncompressed call on uncompressed input, b = g1_inflate_batch -> the uncompressed call -> g1_compress_batch, c = the compressed call" % (WARM, REPS, PROF),
       "rows": {}}
rnd = np.random.RandomState(21)
for kind, conditioned, name, p0, p1, p2, p3 in ROWS:
    committee = kind == "committee"
    if kind == "merge":
        G, n, C, K = p0, p1, p2, p3
        rb, N = (n + 7) // 8, G * C
        cbits = np.zeros((C, n), dtype=bool)
        for c in range(C):
            cbits[c, c * K:(c + 1) * K] = True
        rows = np.ascontiguousarray(np.tile(np.packbits(cbits, axis=1, bitorder="little"), (G, 1)))     # (N, rb)
        csk = np.frombuffer(b"".join((sum(sk_int[c * K:(c + 1) * K]) % R or 1).to_bytes(32, "big") for c in range(C)), dtype=np.uint8).reshape(C, 32)
        grp = np.repeat(np.arange(G), C)
        msg_tab = np.frombuffer(b"".join(synth.msg_of(90000 + g) for g in range(G)), dtype=np.uint8).reshape(G, ML)
        sigs = sign(csk[np.tile(np.arange(C), G)], msg_tab[grp])
        soff = np.arange(G + 1, dtype=np.uint64) * C
        want_rows = np.tile(np.packbits(cbits.any(axis=0), bitorder="little"), G).tobytes()
        row_bytes, wrong = rb * G, 0
        pks = np.ascontiguousarray(pk_all[:n])
    else:
        if committee:
            n, n_com, size, per = p0, p1, p2, p3
            G, part, wrong_every = n_com * per, 2 / 3, 0
            mem2 = np.stack([rnd.permutation(r) for r in np.arange(n_com * size, dtype=np.uint32).reshape(n_com, size)]).astype(np.uint32)
            members = np.ascontiguousarray(mem2.reshape(-1))
            com_off = np.arange(n_com + 1, dtype=np.uint64) * np.uint64(size)
            com = np.repeat(np.arange(n_com, dtype=np.uint32), per)
            width = size
        else:
            G, n, part, wrong_every = p0, p1, p2, p3
            width = n
        bits = np.ones((G, width), dtype=bool) if part >= 1.0 else rnd.random_sample((G, width)) < part
        bits[:, 0] = True; bits[:, 1 % width] = True
        grp, idx = np.nonzero(bits)                                     # entries in group order, indices increasing inside a group
        idx = idx.astype(np.uint32)
        N = len(idx)
        soff = np.zeros(G + 1, dtype=np.uint64)
        soff[1:] = np.cumsum(np.bincount(grp, minlength=G))
        msg_tab = np.frombuffer(b"".join(synth.msg_of(90000 + g) for g in range(G)), dtype=np.uint8).reshape(G, ML)
        # every entry signed by its key on its group's message; the wrong ones by the next key of the sequence
        signer = (mem2[com[grp], idx] if committee else idx).astype(np.int64)
        bad_entries = np.array([int(soff[g]) + 1 for g in range(0, G, wrong_every)] if wrong_every else [], dtype=np.int64)
        signer[bad_entries] += 1
        sigs = sign(sk_all[signer], msg_tab[grp])
        want_bits = bits.copy()
        want_bits[grp[bad_entries], idx[bad_entries]] = False
        want_rows = np.packbits(want_bits, axis=1, bitorder="little").tobytes()
        rb = (width + 7) // 8
        row_bytes, wrong = rb * G, len(bad_entries)
        sel_off = np.arange(G + 1, dtype=np.uint64) * np.uint64(rb)
        pks = np.ascontiguousarray(pk_all[:n])
    moff = np.arange(G + 1, dtype=np.uint64) * ML
    wire = np.zeros(32 * N, dtype=np.uint8)
    assert lib.blsbn254_g1_compress_batch(ctx, P8(sigs), SZ(N), P8(wire)) == 0
    h = ctypes.c_void_p()
    assert lib.blsbn254_keyset_create(ctx, P8(pks), SZ(n), ctypes.byref(h)) == 0
    if committee:
        assert lib.blsbn254_keyset_set_committees(ctx, h, P32(members), P64(com_off), SZ(n_com)) == 0
    res = {k: (np.zeros((32 if k == "c" else 64) * G, dtype=np.uint8), np.zeros(row_bytes, dtype=np.uint8), np.full(G, 0xff, dtype=np.uint8),
               np.zeros((N + 7) // 8 + 1, dtype=np.uint8)) for k in "abc"}
    infl, inf_st, b_wire = np.zeros(64 * N, dtype=np.uint8), np.zeros(N, dtype=np.uint8), np.zeros(32 * G, dtype=np.uint8)

    def call(k, s):
        """the call of this row's kind, compressed for k == 'c', on the signatures s, into res[k]"""
        o, r, st, used = res[k]
        sfx = "_compressed" if k == "c" else ""
        if kind == "merge":
            return getattr(lib, "blsbn254_keyset_merge_checked_batch" + sfx)(ctx, h, P8(rows), P8(s), P64(soff), P8(msg_tab), P64(moff), SZ(G), dst, DL, P8(o), P8(r),
                                                                             P8(used), P8(st))
        if committee:
            return getattr(lib, "blsbn254_keyset_committee_aggregate_checked_batch" + sfx)(ctx, h, P32(com), P32(idx), P8(s), P64(soff), P8(msg_tab), P64(moff),
                                                                                           P64(sel_off), SZ(G), dst, DL, P8(o), P8(r), P8(st))
        return getattr(lib, "blsbn254_keyset_aggregate_checked_batch" + sfx)(ctx, h, P32(idx), P8(s), P64(soff), P8(msg_tab), P64(moff), SZ(G), dst, DL, P8(o), P8(r),
                                                                             P8(st))

    def run_a():
        t = time.perf_counter()
        assert call("a", sigs) == 0
        return (time.perf_counter() - t) * 1e3

    def run_b():
        t = time.perf_counter()
        assert lib.blsbn254_g1_inflate_batch(ctx, P8(wire), SZ(N), P8(infl), P8(inf_st)) == 0
        assert call("b", infl) == 0
        assert lib.blsbn254_g1_compress_batch(ctx, P8(res["b"][0]), SZ(G), P8(b_wire)) == 0
        return (time.perf_counter() - t) * 1e3

    def run_c():
        t = time.perf_counter()
        assert call("c", wire) == 0
        return (time.perf_counter() - t) * 1e3

    forms = (("a", run_a), ("b", run_b), ("c", run_c))
    for _ in range(WARM):
        for _, fn in forms:
            fn()
    for k in "abc":
        assert res[k][2].tobytes() == bytes(G) and res[k][1].tobytes() == want_rows, (name, k)
    assert inf_st.all() and res["b"][0].tobytes() == res["a"][0].tobytes() and res["c"][0].tobytes() == b_wire.tobytes(), name
    times = {k: [] for k in "abc"}
    for _ in range(REPS):
        for k, fn in forms:
            times[k].append(fn())
    row = {"kind": kind, "groups": G, "keys": n, "entries": int(N), "wrong_signatures": int(wrong)}
    for k in "abc":
        row[k] = stats(times[k])
    e.profile_enable(True)
    passes = {k: kernel_passes(fn) for k, fn in forms}
    e.profile_enable(False); e.profile_reset()
    for k in "abc":
        row[k]["kernel_ms"] = {nm: round(float(np.median(v)), 4) for nm, v in sorted(passes[k].items()) if np.median(v) > 0.002}
    a, b, c = row["a"], row["b"], row["c"]
    row["c_over_a"] = round(c["median_ms"] / a["median_ms"], 3)
    row["c_over_b"] = round(c["median_ms"] / b["median_ms"], 3)
    if conditioned:
        row["wall_condition_met"] = bool(c["median_ms"] + c["spread_ms"] + b["spread_ms"] < b["median_ms"])
    scan = "kca_scan" if committee else "ka_scan"
    if kind != "merge":
        # the fused scan of c against the staged form: the inflation of b's first step plus the scan of a, pass by pass
        fused = np.array(passes["c"][scan + "_wire"])
        staged = np.array(passes["b"]["g1_inflate"]) + np.array(passes["a"][scan])
        sp = lambda v: round(float(np.percentile(v, 75) - np.percentile(v, 25)), 4)
        row["scan"] = {"fused_ms": round(float(np.median(fused)), 4), "fused_spread_ms": sp(fused), "staged_ms": round(float(np.median(staged)), 4),
                       "staged_spread_ms": sp(staged), "g1_inflate_ms": round(float(np.median(passes["b"]["g1_inflate"])), 4),
                       "scan_ms": round(float(np.median(passes["a"][scan])), 4)}
        row["scan"]["fused_stays"] = bool(row["scan"]["fused_ms"] <= row["scan"]["staged_ms"] + row["scan"]["fused_spread_ms"] + row["scan"]["staged_spread_ms"])
    out["rows"][name] = row
    lib.blsbn254_keyset_destroy(h)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    open(args.out, "w").write(json.dumps(out, indent=1) + "\n")          # after every row: a run that is cut short keeps what it measured
    print(name, json.dumps(row), flush=True)
e.close()
print(json.dumps(out, indent=1))
