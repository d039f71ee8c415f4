"""What the try-and-increment map to G1 costs, and which form of its search is worth shipping: n = 262 144 32-byte digests over a
pool of 1024 keys on one GPU, signed and verified under SVDW and under TAI_DIGEST (blsbn254_set_g1_map), the forms interleaved
round by round in one process.  Three hash launches are timed with the engine's HIP-event profile inside verify_batch (the
homogeneous form, mode 3): k_hash_to_g1 under SVDW -- the parent commit's kernel, the yardstick, in the same run --, and
k_hash_to_g1_tai with the plain and with the pooled search.  The library holds ONE form of the search (Makefile TAI_FLAGS), so
the other comes from a second build of the same sources loaded beside it:
    make -C bls-bn254_amd VARIANT=_taiplain TAI_FLAGS='-DBN_FORCE_INLINE -DBN_WAVES_PER_SIMD=2 -DTAI_PLAIN'
(--other names it, --other-form says which form it holds).  Also: the wall time of verify_batch under SVDW and under the shipped
TAI form, and the rounds a wave runs -- a round is one Jacobi symbol for the whole wave -- under either form.  The rounds are a
function of the digests alone, so they are REPLAYED on the CPU over this run's digests by the two rules (plain: 1 + the longest
run among the wave's 64 messages; pooled: the dealing rule of k_hash_tai.hip), before the GPU is opened; they are exact for this
input, not sampled from the device.
Usage: python scripts/bench_g1_map.py [--out profiles/g1_map.json] [--n 262144] [--reps 7] [--other PATH --other-form plain] -> JSON"""
import argparse, concurrent.futures, json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
from tests import g1_map_support as G
from tests import synth

SHIPPED_FORM = "pooled"         # the search the library is built with (bls-bn254_amd/Makefile TAI_FLAGS)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join("profiles", "g1_map.json"))
ap.add_argument("--n", type=int, default=262144)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--other", default=os.path.join("bls-bn254_amd", "libblsbn254_hip_taiplain.so"))
ap.add_argument("--other-form", default="plain", choices=("plain", "pooled"))
args = ap.parse_args()
assert args.other_form != SHIPPED_FORM
N, POOL, REPS, WARM, PROF = args.n, 1024, max(args.reps, 1), 2, 7


def runs_of(lo_hi):
    return [G.run_of(int.from_bytes(synth.msg_of(i), "big") % G.P) for i in range(*lo_hi)]


def pooled_rounds(runs):
    """the rounds of tai_search_pooled for one wave: round 1 tests candidate 0 of every message; then the u open messages get
    64 // u lanes each, and `done` candidates per open message are known non-residues"""
    rounds, done, open_ = 1, 1, [r for r in runs if r >= 1]
    while open_:
        per = 64 // len(open_)
        done += per; rounds += 1
        open_ = [r for r in open_ if r >= done]
    return rounds


def replay():
    step = 4096
    with concurrent.futures.ProcessPoolExecutor(14) as ex:                   # before the GPU is opened: workers never see it
        runs = [r for part in ex.map(runs_of, [(lo, min(lo + step, N)) for lo in range(0, N, step)]) for r in part]
    waves = [runs[lo:lo + 64] for lo in range(0, N, 64)]
    plain = [1 + max(w) for w in waves]
    pooled = [pooled_rounds(w) for w in waves]
    return {"candidates_per_message_mean": round(1 + float(np.mean(runs)), 4), "longest_run": int(max(runs)), "waves": len(waves),
            "plain": {"mean": round(float(np.mean(plain)), 3), "max": int(max(plain))},
            "pooled": {"mean": round(float(np.mean(pooled)), 3), "max": int(max(pooled))}}


if __name__ == "__main__":
    rounds = replay()
    import blsbn254_loader; M = blsbn254_loader.load()
    dst = M.DEFAULT_DST
    e = M.Engine(0)
    # a second build of the same library beside the first: every Engine keeps the library it was created from
    os.environ["BLSBN254_LIB"] = os.path.abspath(args.other)
    M.engine._lib = None
    other = M.Engine(0)
    assert other._lib is not e._lib
    pool = min(POOL, N)
    skb = b"".join(synth.sk_of(k).to_bytes(32, "big") for k in range(pool))
    pk_pool = e.sk_to_pk_batch(skb, pool)
    pks = pk_pool * (N // pool) + pk_pool[:128 * (N % pool)]
    sk_all = skb * (N // pool) + skb[:32 * (N % pool)]
    msgs = [synth.msg_of(i) for i in range(N)]
    ones = synth.bitmap_of([True] * N)
    sigs = {G.SVDW: e.sign_batch(sk_all, msgs, dst)}
    e.set_g1_map(G.TAI_DIGEST); other.set_g1_map(G.TAI_DIGEST)
    sigs[G.TAI_DIGEST] = e.sign_batch(sk_all, msgs, dst)
    assert other.sign_batch(sk_all[:32 * 8192], msgs[:8192], dst) == sigs[G.TAI_DIGEST][:64 * 8192], "the two forms of the search disagree"
    assert e.hash_to_g1_batch(msgs[:256], dst) == b"".join(G.hash_bytes(G.TAI_DIGEST, 0, m) for m in msgs[:256])
    assert e.verify_batch(pks[:128 * 4096], msgs[:4096], sigs[G.SVDW][:64 * 4096], dst) == bytes(512)            # SVDW signatures under TAI
    FORMS = {"svdw": (e, G.SVDW), "tai_" + SHIPPED_FORM: (e, G.TAI_DIGEST), "tai_" + args.other_form: (other, G.TAI_DIGEST)}

    def stats(v):
        a = np.sort(np.array(v))
        return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a[0]), 4), "max_ms": round(float(a[-1]), 4), "reps": len(v)}

    def verify(form):
        eng, map_id = FORMS[form]
        eng.set_g1_map(map_id)                              # outside the timed region
        t = time.perf_counter()
        bm = eng.verify_batch(pks, msgs, sigs[map_id], dst)
        ms = (time.perf_counter() - t) * 1e3
        assert bm == ones, form
        return ms

    wall = {f: [] for f in FORMS}
    for r in range(WARM + REPS):
        for f in FORMS:
            ms = verify(f)
            if r >= WARM:
                wall[f].append(ms)
    hash_ms, launches = {f: [] for f in FORMS}, {}
    e.profile_enable(True); other.profile_enable(True)
    for _ in range(PROF):
        for f in FORMS:
            FORMS[f][0].profile_reset()
            verify(f)
            rec = FORMS[f][0].profile_read()["hash_to_g1"]
            hash_ms[f].append(rec["total_ms"]); launches[f] = rec["launches"]
    for x in (e, other):
        x.profile_enable(False); x.profile_reset(); x.close()
    base_w, base_h = np.median(wall["svdw"]), np.median(hash_ms["svdw"])
    out = {"method": "one process, two contexts on one GPU (the library and a second build of it holding the other form of the search), the forms "
                     "interleaved round by round; verify_batch: host clock around the call (host pointers, ends synchronised), %d warm-up + %d timed "
                     "rounds; hash_to_g1: the HIP-event profile's total for the hash-to-G1 launches of one verify_batch (homogeneous output, mode 3), "
                     "%d further rounds; ratios are medians over the median under SVDW (the parent commit's kernel) of the same run; rounds_per_wave: "
                     "replayed on the CPU over the same digests, exact for this input" % (WARM, REPS, PROF),
           "n": N, "keys": pool, "message_bytes": 32, "shipped_form": SHIPPED_FORM, "rounds_per_wave": rounds, "forms": {}}
    for f in FORMS:
        row = {"hash_to_g1": dict(stats(hash_ms[f]), launches=launches[f], over_svdw=round(float(np.median(hash_ms[f]) / base_h), 3)),
               "verify_batch": dict(stats(wall[f]), over_svdw=round(float(np.median(wall[f]) / base_w), 3))}
        out["forms"][f] = row
    p, q = hash_ms["tai_plain"], hash_ms["tai_pooled"]
    out["pooled_vs_plain"] = {"hash_to_g1_median_ratio": round(float(np.median(q) / np.median(p)), 3),
                              "ranges_overlap": bool(min(q) <= max(p) and min(p) <= max(q))}
    out["tai_not_slower_than_svdw"] = bool(np.median(hash_ms["tai_" + SHIPPED_FORM]) <= base_h)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    open(args.out, "w").write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out, indent=1))
