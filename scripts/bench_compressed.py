"""The calls on compressed operands against the calls they replace, on identical inputs, all through the C ABI on numpy buffers:
  verify    (a) blsbn254_verify_batch on uncompressed input
            (b) the composition the uncompressed API forces on a caller holding wire bytes: blsbn254_g1_decompress_batch +
                blsbn254_g2_decompress_batch (results to the host) + blsbn254_verify_batch (uploads them again)
            (c) blsbn254_verify_batch_compressed
  register  blsbn254_keyset_create against blsbn254_keyset_create_compressed
  keyset    blsbn254_keyset_fast_aggregate_verify_batch against its _compressed form
Per row: warm-up, REPS timed repetitions of each form, alternating; median, quartiles, min and max of the wall time (host clock
around calls that end synchronised).  Kernel times of k_g1/g2_inflate and of k_g1/g2_codec in decompress mode at the same n come
from the engine's HIP-event profile in passes of their own.  Every form is checked to give the expected bitmap.
Usage: python scripts/bench_compressed.py [--out profiles/compressed.json] [--reps 12] [--quick] -> JSON"""
import argparse, ctypes, json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import blsbn254_loader; M = blsbn254_loader.load()
from tests import synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join("profiles", "compressed.json"))
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--quick", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
args = ap.parse_args()
REPS, WARM, PROF = max(args.reps, 1), 2, 3
POOL, SHAPES, REG_KEYS, KS_KEYS, KS_GROUPS = 1024, [262144, 1024], 65536, 1024, 4096
if args.quick:
    POOL, SHAPES, REG_KEYS, KS_KEYS, KS_GROUPS = 16, [300], 200, 70, 40
u8, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
P8 = lambda a: a.ctypes.data_as(u8)
P64 = lambda a: a.ctypes.data_as(u64)
SZ = ctypes.c_size_t
dst = M.DEFAULT_DST
e = M.Engine(0)
lib, ctx = e._lib, e._ctx
R = synth.R
arr = lambda b: np.frombuffer(b, dtype=np.uint8).copy()
b32 = lambda v: int(v).to_bytes(32, "big")


def stats(ms):
    a = np.sort(np.array(ms))
    q1, med, q3 = (float(np.percentile(a, p)) for p in (25, 50, 75))
    return {"median_ms": round(med, 3), "spread_ms": round(q3 - q1, 3), "q1_ms": round(q1, 3), "q3_ms": round(q3, 3), "min_ms": round(float(a[0]), 3),
            "max_ms": round(float(a[-1]), 3), "reps": len(ms)}


def below(a, b):
    """a's median lies below b's by more than the two spreads together"""
    return bool(a["median_ms"] + a["spread_ms"] + b["spread_ms"] < b["median_ms"])


def timed(fn):
    t = time.perf_counter()
    rc = fn()
    dt = time.perf_counter() - t
    assert rc == 0, rc
    return dt * 1e3


def race(forms):
    """forms: [(name, fn)] -> {name: stats}, alternating"""
    for _ in range(WARM):
        for _, fn in forms:
            timed(fn)
    times = {k: [] for k, _ in forms}
    for _ in range(REPS):
        for k, fn in forms:
            times[k].append(timed(fn))
    return {k: stats(v) for k, v in times.items()}


def kernel_ms(fn, names):
    e.profile_enable(True); e.profile_reset()
    for _ in range(PROF):
        assert fn() == 0
    pr = e.profile_read()
    e.profile_enable(False); e.profile_reset()
    return {n: round(pr[n]["total_ms"] / PROF, 4) for n in names}


out = {"method": "wall: host clock around C-ABI calls that end synchronised, %d warm-up + %d timed repetitions per form, alternating; spread = interquartile "
                 "range; kernel_ms: HIP-event profile, mean of %d further repetitions in passes of their own" % (WARM, REPS, PROF),
       "verify": {}, "register": {}, "keyset": {}}
NMAX = max(POOL, REG_KEYS, KS_KEYS)
sks = [synth.sk_of(k) for k in range(NMAX)]
skb = b"".join(map(b32, sks))
pk_all = e.sk_to_pk_batch(skb, NMAX)
pkc_all = e.g2_compress_batch(pk_all, NMAX)

# ---- verify
for n in SHAPES:
    msgs = [synth.msg_of(i) for i in range(n)]
    bad = set(range(999 % n, n, 1000))
    signed = [b"not this tuple's message" if i in bad else m for i, m in enumerate(msgs)]
    reps_, rem = divmod(n, POOL)
    sigs = arr(e.sign_batch(skb[:32 * POOL] * reps_ + skb[:32 * rem], signed, dst))
    pks = arr(pk_all[:128 * POOL] * reps_ + pk_all[:128 * rem])
    pks_c = arr(pkc_all[:64 * POOL] * reps_ + pkc_all[:64 * rem])
    sigs_c = arr(e.g1_compress_batch(sigs, n))
    data, off = M.engine.pack_messages(msgs)
    data = arr(data)
    want = synth.bitmap_of([i not in bad for i in range(n)])
    nb = (n + 7) // 8
    bm = {k: np.zeros(nb, dtype=np.uint8) for k in "abc"}
    tmp_pk, tmp_sig = np.zeros(128 * n, dtype=np.uint8), np.zeros(64 * n, dtype=np.uint8)
    st = np.zeros(n, dtype=np.uint8)

    def run_a():
        return lib.blsbn254_verify_batch(ctx, P8(pks), P8(data), P64(off), P8(sigs), SZ(n), dst, SZ(len(dst)), P8(bm["a"]))

    def run_b():
        rc = lib.blsbn254_g1_decompress_batch(ctx, P8(sigs_c), SZ(n), P8(tmp_sig)) or lib.blsbn254_g2_decompress_batch(ctx, P8(pks_c), SZ(n), P8(tmp_pk))
        return rc or lib.blsbn254_verify_batch(ctx, P8(tmp_pk), P8(data), P64(off), P8(tmp_sig), SZ(n), dst, SZ(len(dst)), P8(bm["b"]))

    def run_c():
        return lib.blsbn254_verify_batch_compressed(ctx, P8(pks_c), P8(data), P64(off), P8(sigs_c), SZ(n), dst, SZ(len(dst)), P8(bm["c"]))

    row = race([("a_uncompressed", run_a), ("b_decompress_then_verify", run_b), ("c_compressed", run_c)])
    assert all(v.tobytes() == want for v in bm.values()), n
    row["kernel_ms"] = kernel_ms(lambda: lib.blsbn254_g1_inflate_batch(ctx, P8(sigs_c), SZ(n), P8(tmp_sig), P8(st))
                                 or lib.blsbn254_g2_inflate_batch(ctx, P8(pks_c), SZ(n), P8(tmp_pk), P8(st))
                                 or lib.blsbn254_g1_decompress_batch(ctx, P8(sigs_c), SZ(n), P8(tmp_sig))
                                 or lib.blsbn254_g2_decompress_batch(ctx, P8(pks_c), SZ(n), P8(tmp_pk)), ("g1_inflate", "g2_inflate", "g1_codec", "g2_codec"))
    row["c_below_b"] = below(row["c_compressed"], row["b_decompress_then_verify"])
    row["c_over_a"] = round(row["c_compressed"]["median_ms"] / row["a_uncompressed"]["median_ms"], 3)
    row["c_minus_a_ms"] = round(row["c_compressed"]["median_ms"] - row["a_uncompressed"]["median_ms"], 3)
    row["c_over_b"] = round(row["c_compressed"]["median_ms"] / row["b_decompress_then_verify"]["median_ms"], 3)
    row["tuples"], row["key_pool"] = n, min(POOL, n)
    out["verify"]["%d tuples over %d keys" % (n, min(POOL, n))] = row

# ---- registration
reg_pk, reg_pkc = arr(pk_all[:128 * REG_KEYS]), arr(pkc_all[:64 * REG_KEYS])


def create(compressed):
    h = ctypes.c_void_p()
    if compressed:
        rc = lib.blsbn254_keyset_create_compressed(ctx, P8(reg_pkc), None, SZ(REG_KEYS), None, SZ(0), ctypes.byref(h))
    else:
        rc = lib.blsbn254_keyset_create(ctx, P8(reg_pk), SZ(REG_KEYS), ctypes.byref(h))
    create.h = h
    return rc


def create_and_destroy(compressed):
    t = timed(lambda: create(compressed))
    lib.blsbn254_keyset_destroy(create.h)
    return t


for _ in range(WARM):
    create_and_destroy(False); create_and_destroy(True)
tt = {"uncompressed": [], "compressed": []}
for _ in range(REPS):
    tt["uncompressed"].append(create_and_destroy(False)); tt["compressed"].append(create_and_destroy(True))
row = {k: stats(v) for k, v in tt.items()}
row["keys"] = REG_KEYS
row["compressed_over_uncompressed"] = round(row["compressed"]["median_ms"] / row["uncompressed"]["median_ms"], 3)
out["register"]["%d keys" % REG_KEYS] = row

# ---- key-set verify
rnd = np.random.RandomState(13)
G, n = KS_GROUPS, KS_KEYS
bits = rnd.random_sample((G, n)) < 2 / 3
bits[:, 0] = True
rows = np.packbits(bits, axis=1, bitorder="little")
ska = np.array(sks[:n], dtype=object)
agg = [int(sum(ska[bits[g]])) % R or 1 for g in range(G)]
msgs = [synth.msg_of(90000 + g) for g in range(G)]
sigs = arr(e.sign_batch(b"".join(map(b32, agg)), msgs, dst))
sigs_c = arr(e.g1_compress_batch(sigs, G))
data, off = M.engine.pack_messages(msgs)
data = arr(data)
h = ctypes.c_void_p()
ks_pkc = arr(pkc_all[:64 * n])
assert lib.blsbn254_keyset_create_compressed(ctx, P8(ks_pkc), None, SZ(n), None, SZ(0), ctypes.byref(h)) == 0
bm_u, bm_c = np.zeros((G + 7) // 8, dtype=np.uint8), np.zeros((G + 7) // 8, dtype=np.uint8)
row = race([("uncompressed", lambda: lib.blsbn254_keyset_fast_aggregate_verify_batch(ctx, h, P8(rows), P8(data), P64(off), P8(sigs), SZ(G), dst, SZ(len(dst)), P8(bm_u))),
            ("compressed", lambda: lib.blsbn254_keyset_fast_aggregate_verify_batch_compressed(ctx, h, P8(rows), P8(data), P64(off), P8(sigs_c), SZ(G), dst, SZ(len(dst)),
                                                                                              P8(bm_c)))])
assert bm_u.tobytes() == bm_c.tobytes() == synth.bitmap_of([True] * G)
lib.blsbn254_keyset_destroy(h)
row["groups"], row["keys"] = G, n
row["compressed_over_uncompressed"] = round(row["compressed"]["median_ms"] / row["uncompressed"]["median_ms"], 3)
out["keyset"]["%d groups over %d keys at 2/3" % (G, n)] = row

e.close()
text = json.dumps(out, indent=1)
os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
open(args.out, "w").write(text + "\n")
print(text)
