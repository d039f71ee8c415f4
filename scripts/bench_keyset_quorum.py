"""FastAggregateVerify with a quorum over a registered key set (blsbn254_keyset_quorum_verify_batch) against the composition the
parent API offers on the same inputs: blsbn254_keyset_fast_aggregate_verify_batch on ALL groups, plus the weighing on the host with
numpy (unpackbits, a masked 64-bit sum per column, the quorum rule, the AND with the bitmap).  Both through the C ABI on numpy
buffers.  Per row: warm-up, REPS timed repetitions of each form, alternating; median, quartiles, min and max of the wall time
(host clock around calls that end synchronised).  The parent's verify call alone is the first part of every composition run and
is reported too: new call minus that = what the weighing and its synchronisation cost on the all-reach rows.  Kernel times come
from the engine's HIP-event profile in passes of their own.  Also: blsbn254_keyset_set_weights, and the registration with proofs
against blsbn254_keyset_create plus blsbn254_pop_verify_batch for 1024 keys.
Usage: python scripts/bench_keyset_quorum.py [--out profiles/keyset_quorum.json] [--reps 20] [--quick] -> JSON"""
import argparse, ctypes, json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import blsbn254_loader; M = blsbn254_loader.load()
from tests import synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join("profiles", "keyset_quorum.json"))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--quick", action="store_true", help="tiny rows: a rehearsal of the script, not a measurement")
args = ap.parse_args()
REPS, WARM, PROF = max(args.reps, 1), 3, 3
# groups, keys, columns, participation, fraction of the groups at 1/4 participation (below quorum), name
ROWS = [(4096, 1024, 1, 2 / 3, 0.0, "4096 groups, 1024 keys, 2/3 participation, 1 column, all reach"),
        (4096, 1024, 4, 2 / 3, 0.0, "4096 groups, 1024 keys, 2/3 participation, 4 columns, all reach"),
        (4096, 1024, 1, 2 / 3, 0.5, "4096 groups, 1024 keys, half at 1/4 participation and below quorum, 1 column"),
        (4096, 1024, 4, 2 / 3, 0.5, "4096 groups, 1024 keys, half at 1/4 participation and below quorum, 4 columns"),
        (4096, 64, 1, 1.0, 0.0, "4096 groups, 64 keys, all selected, 1 column"), (16, 64, 1, 1.0, 0.0, "16 groups, 64 keys, all selected, 1 column")]
NREG = 1024
if args.quick:
    ROWS = [(24, 70, 1, 2 / 3, 0.0, "quick all reach"), (24, 70, 4, 2 / 3, 0.5, "quick half below")]
    NREG = 70
u8, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
P8 = lambda a: a.ctypes.data_as(u8)
P64 = lambda a: a.ctypes.data_as(u64)
dst = M.DEFAULT_DST
e = M.Engine(0)
lib, ctx = e._lib, e._ctx
R = synth.R
NMAX = max(max(r[1] for r in ROWS), NREG)
sks = np.array([synth.sk_of(k) for k in range(NMAX)], dtype=object)
sk_bytes = b"".join(int(s).to_bytes(32, "big") for s in sks)
pk_all = np.frombuffer(e.sk_to_pk_batch(sk_bytes, NMAX), dtype=np.uint8).reshape(NMAX, 128)


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
rnd = np.random.RandomState(11)
for G, n, nc, part, frac_low, name in ROWS:
    pks = np.ascontiguousarray(pk_all[:n])
    bits = np.ones((G, n), dtype=bool) if part >= 1.0 else rnd.random_sample((G, n)) < part
    low = np.zeros(G, dtype=bool)
    if frac_low:
        low[rnd.permutation(G)[:int(G * frac_low)]] = True
        bits[low] = rnd.random_sample((int(low.sum()), n)) < 0.25
    bits[:, 0] = True
    sel = np.packbits(bits, axis=1, bitorder="little")                 # G rows of ceil(n / 8) bytes, LSB-first
    agg = [int(sum(sks[:n][bits[g]])) % R or 1 for g in range(G)]
    msgs = [synth.msg_of(50000 + g) for g in range(G)]
    sigs = np.frombuffer(e.sign_batch(b"".join(s.to_bytes(32, "big") for s in agg), msgs, dst), dtype=np.uint8)
    for g in range(6, G, 7):
        msgs[g] = bytes([msgs[g][0] ^ 1]) + msgs[g][1:]
    data, off = M.engine.pack_messages(msgs)
    data = np.frombuffer(data, dtype=np.uint8)
    nb = (G + 7) // 8
    wts = np.ascontiguousarray(rnd.randint(1, 1 << 40, size=(nc, n)).astype(np.uint64))
    min_w = np.ascontiguousarray(wts.sum(axis=1) // np.uint64(2))      # half of each column's stake: 2/3 reaches, 1/4 does not
    want_w = np.stack([np.sum(np.broadcast_to(wts[q], (G, n)), axis=1, where=bits) for q in range(nc)], axis=1)
    reach = (want_w >= min_w).all(axis=1)
    assert reach.sum() == G - low.sum() and not reach[low].any(), name
    want = synth.bitmap_of([bool(reach[g]) and g % 7 != 6 for g in range(G)])
    bm_new, bm_old, w_new = np.zeros(nb, dtype=np.uint8), np.zeros(nb, dtype=np.uint8), np.zeros((G, nc), dtype=np.uint64)
    h = ctypes.c_void_p()
    assert lib.blsbn254_keyset_create(ctx, P8(pks), ctypes.c_size_t(n), ctypes.byref(h)) == 0
    t_set = []
    for _ in range(WARM + REPS):
        t = time.perf_counter()
        assert lib.blsbn254_keyset_set_weights(ctx, h, P64(wts), ctypes.c_size_t(nc)) == 0
        t_set.append((time.perf_counter() - t) * 1e3)

    def run_new():
        t = time.perf_counter()
        rc = lib.blsbn254_keyset_quorum_verify_batch(ctx, h, P8(sel), P8(data), P64(off), P8(sigs), ctypes.c_size_t(G), dst, ctypes.c_size_t(len(dst)),
                                                     P64(min_w), P64(w_new), P8(bm_new))
        dt = time.perf_counter() - t
        assert rc == 0
        return dt * 1e3, 0.0

    comp = {}

    def run_old():
        t = time.perf_counter()
        rc = lib.blsbn254_keyset_fast_aggregate_verify_batch(ctx, h, P8(sel), P8(data), P64(off), P8(sigs), ctypes.c_size_t(G), dst, ctypes.c_size_t(len(dst)),
                                                             P8(bm_old))
        tv = time.perf_counter()
        mask = np.unpackbits(sel, axis=1, count=n, bitorder="little").view(bool)      # the weighing a caller of the parent API does
        w = np.stack([np.sum(np.broadcast_to(wts[q], (G, n)), axis=1, where=mask) for q in range(nc)], axis=1)
        ok = (w >= min_w).all(axis=1)
        comp["bm"] = np.packbits(ok, bitorder="little") & bm_old
        comp["w"] = w
        dt = time.perf_counter() - t
        assert rc == 0
        return dt * 1e3, (tv - t) * 1e3

    for _ in range(WARM):
        run_new(); run_old()
    assert bm_new.tobytes() == want and comp["bm"].tobytes() == want, name
    assert (w_new == want_w).all() and (comp["w"] == want_w).all(), name
    t_new, t_old, t_parent = [], [], []
    for _ in range(REPS):
        t_new.append(run_new()[0])
        o = run_old(); t_old.append(o[0]); t_parent.append(o[1])
    row = {"groups": G, "keys": n, "columns": nc, "selected_keys": int(bits.sum()), "groups_below_quorum": int(low.sum()), "quorum": stats(t_new),
           "composition": stats(t_old), "parent_verify_alone": stats(t_parent), "set_weights": stats(t_set[WARM:])}
    row["composition_host_weighing_median_ms"] = round(float(np.median(np.array(t_old) - np.array(t_parent))), 3)
    row["quorum_minus_parent_verify_median_ms"] = round(row["quorum"]["median_ms"] - row["parent_verify_alone"]["median_ms"], 3)
    e.profile_enable(True)
    for key, fn in (("quorum", run_new), ("composition", run_old)):
        e.profile_reset()
        for _ in range(PROF):
            fn()
        row[key]["kernel_ms"] = kernels(PROF)
    e.profile_enable(False); e.profile_reset()
    row["ks_weight_kernel_ms"] = row["quorum"]["kernel_ms"].get("ks_weight", 0.0)
    row["below_composition"] = below(row["quorum"], row["composition"])
    if frac_low:
        row["below_parent_verify_alone"] = below(row["quorum"], row["parent_verify_alone"])
    out["rows"][name] = row
    lib.blsbn254_keyset_destroy(h)

# registration: with proofs, against the plain registration plus the proofs' verification
pks = np.ascontiguousarray(pk_all[:NREG])
proofs = np.frombuffer(e.pop_prove_batch(sk_bytes[:32 * NREG], NREG), dtype=np.uint8)
tag = M.POP_DST
bm = np.zeros((NREG + 7) // 8, dtype=np.uint8)


def reg_checked():
    h = ctypes.c_void_p()
    t = time.perf_counter()
    rc = lib.blsbn254_keyset_create_checked(ctx, P8(pks), P8(proofs), ctypes.c_size_t(NREG), tag, ctypes.c_size_t(len(tag)), ctypes.byref(h))
    dt = time.perf_counter() - t
    assert rc == 0
    assert lib.blsbn254_keyset_valid(ctx, h, P8(bm)) == 0 and bm.tobytes() == synth.bitmap_of([True] * NREG)
    lib.blsbn254_keyset_destroy(h)
    return dt * 1e3


def reg_plain():
    h = ctypes.c_void_p()
    t = time.perf_counter()
    rc = lib.blsbn254_keyset_create(ctx, P8(pks), ctypes.c_size_t(NREG), ctypes.byref(h))
    rc2 = lib.blsbn254_pop_verify_batch(ctx, P8(pks), P8(proofs), ctypes.c_size_t(NREG), tag, ctypes.c_size_t(len(tag)), P8(bm))
    dt = time.perf_counter() - t
    assert rc == 0 and rc2 == 0 and bm.tobytes() == synth.bitmap_of([True] * NREG)
    lib.blsbn254_keyset_destroy(h)
    return dt * 1e3


for _ in range(WARM):
    reg_checked(); reg_plain()
t_c, t_p = [], []
for _ in range(REPS):
    t_c.append(reg_checked()); t_p.append(reg_plain())
out["registration"] = {"keys": NREG, "keyset_create_checked": stats(t_c), "keyset_create + pop_verify_batch": stats(t_p)}
e.close()
text = json.dumps(out, indent=1)
os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
open(args.out, "w").write(text + "\n")
print(text)
