"""GPU tests (MI355X) of what a context keeps BETWEEN calls: the resident domain-separation tag, the queue of unsettled
verify_batch_dev calls, the remembered key count, prepared-key tables and de-duplication buffers, workspaces that only grow,
the second stream, the forced MSM window.  A result that depends on what the context did before is a wrong result.

A. Directed: a verify_batch_dev call that names a new tag right behind a pending call whose key-count guess fails.  The pending
   call's re-run stages ITS tag; if that happens between the staging of the new tag and the new call's kernels, the new call
   hashes under the old tag ("Ordering rule of the asynchronous path").
B. Seeded sequences over a table of operations of every family that touches shared state: each operation's bytes on ONE
   long-lived context must equal its bytes on a context of its own, which are checked against the CPU oracle / closed forms.
C. The first sequence on two contexts of one GPU, interleaved step by step: each gives the bytes it gives alone.

Expected values never come from the context under test.  No bitmap of a pending call is read before synchronize() or a
following entry point has returned."""
import random
import time

import numpy as np
import pytest

from tests import synth
from tests.gpu_support import eng, M
from tests.helpers import b32

pytestmark = pytest.mark.gpu
ONE_GT = (1).to_bytes(32, "big") + bytes(352)
R = synth.R


def popcount(bm):
    return int(np.unpackbits(np.frombuffer(bm, dtype=np.uint8)).sum())


def bit(bm, i):
    return bm[i >> 3] >> (i & 7) & 1


def sample_of(n, seed):
    """every index up to a few hundred elements; beyond that the first, the last and 16 seeded ones"""
    if n <= 300:
        return list(range(n))
    return sorted({0, n - 1} | set(random.Random(seed).sample(range(n), 16)))


def tags_of(M):
    d = M.DEFAULT_DST
    assert len(d) == 40
    long_ = b"BLSBN254-ctx-sequence-tag:" * 12
    return {"0": b"", "1": b"Q", "40": d, "40b": d[:-1] + bytes([d[-1] ^ 1]), "255": long_[:255], "255b": long_[:254] + b"#",
            "256": long_[:256], "300": long_[:300]}


def run_dev(e, t, n, tag, bm, rlc=False):
    (e.verify_batch_rlc_dev if rlc else e.verify_batch_dev)(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), n, bm.data_ptr(), tag)


# ================================================================ A. tag change across a re-run

# How long the context's stream is held before batch B may start.  B's pending event must not have fired when C enters: the
# non-blocking settle at C's entry would re-run B before C stages its tag, which is the harmless order.  Measured on an MI355X
# with the parent commit's library (three runs, host clock around call .. synchronize): batch B (16000 tuples, 5000 keys)
# takes 7.5 ms when its guess holds and 12.7 - 13.2 ms with its re-run; the host needs 0.1 - 0.3 ms from the call of B to the
# call of C, three calls of A in between included (printed by the test itself).  100 ms is more than seven times the longest
# of these, and leaves room for a host that is descheduled between two calls.  The test asserts that the hold was still
# running just before C was called, so a hold that was too short shows as an error of the test and never as a pass.
HOLD_MS = 100.0


def hold_stream(torch, e, ms):
    """Bounded GPU work on the context's own stream: a fixed-length spin, its length calibrated with device events.  Returns an
    event behind the spin."""
    s = torch.cuda.ExternalStream(e.stream, device=torch.device("cuda", 0))
    probe = 2000000
    with torch.cuda.stream(s):
        torch.cuda._sleep(1000)                       # loads the spin kernel
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(s); torch.cuda._sleep(probe); t1.record(s)
        t1.synchronize()
        probe_ms = t0.elapsed_time(t1)
        assert 0.05 < probe_ms < 500.0, "calibration of the spin is off: %d cycles took %.3f ms" % (probe, probe_ms)
        torch.cuda._sleep(int(ms * probe / probe_ms))  # bounded: at most ms / 0.05 probes
        done = torch.cuda.Event()
        done.record(s)
    return done


_A_BATCHES = {}


def _a_batch(eng, oracle, key, *args, **kw):
    if key not in _A_BATCHES:
        _A_BATCHES[key] = synth.make_batch_gpu(eng, oracle, *args, spot=6, **kw)
    return _A_BATCHES[key]


@pytest.mark.parametrize("direction", ["signed_under_tag2", "signed_under_tag1"])
@pytest.mark.parametrize("trigger", ["oversize_tag", "two_chunks", "five_in_flight"])
def test_tag_change_behind_a_failing_guess(eng, oracle, M, monkeypatch, trigger, direction):
    """Batch A (tag 1, 40 keys) twice, so the context enqueues on a guess of 40 keys.  Batch B (tag 1, 5000 keys: more than the
    capacity of 1024) is enqueued behind a bounded hold of the stream, so its check cannot have come back when batch C enters
    with tag 2.  C reaches a blocking settle of B by one of three ways: a tag of 300 bytes (not eligible for the asynchronous
    path), more tuples than one chunk, or a full queue of four.  C's bitmap must be the one tag 2 gives: the closed form when C
    was signed under tag 2, all zero when it was signed under tag 1 (tag 2 then has tag 1's length and differs in one byte,
    except for the 300-byte tag, which is hashed down to 32 bytes and keeps that direction as a plain negative case).

    Against the library before the ordering fix (C's popcount expected / observed): oversize tag 3645 / 0 and 0 / 0 (the negative
    case cannot tell), two chunks 17778 / 0 and 0 / 17778, five in flight 3645 / 0 and 0 / 3645: five of the six cases fail."""
    import torch
    T = tags_of(M)
    tag1 = T["40"]
    tag2 = T["300"] if trigger == "oversize_tag" else T["40b"]
    assert trigger == "oversize_tag" or (len(tag2) == len(tag1) and sum(x != y for x, y in zip(tag1, tag2)) == 1)
    nA, nB = 16000, 16000          # A as long as B: B must not grow a workspace (freeing the old one waits for the device, the hold included)
    nC = 20000 if trigger == "two_chunks" else 4100
    if trigger == "two_chunks":
        monkeypatch.setenv("BLSBN254_CHUNK_LANES", "16384")
    A = _a_batch(eng, oracle, "A", nA, tag1, pool=40, invalid_every=7)
    B = _a_batch(eng, oracle, "B", nB, tag1, pool=5000, invalid_every=11, base=100000)
    if direction == "signed_under_tag2":
        C = _a_batch(eng, oracle, ("C", nC, tag2), nC, tag2, pool=40, invalid_every=9, base=200000)
        wantC = synth.bitmap_of(C[3])
        assert 0 < popcount(wantC) < nC
    else:
        C = _a_batch(eng, oracle, ("C", nC, tag1), nC, tag1, pool=40, invalid_every=9, base=200000)
        wantC = bytes((nC + 7) // 8)
    wantA, wantB = synth.bitmap_of(A[3]), synth.bitmap_of(B[3])
    e = M.Engine(0)
    try:
        tA, tB, tC = (synth.dev_batch(M, torch, x[0], x[1], x[2]) for x in (A, B, C))
        extra = [torch.full_like(tA[4], 0x5a) for _ in range(3)]
        torch.cuda.synchronize()
        run_dev(e, tA, nA, tag1, tA[4]); e.synchronize()
        assert bytes(tA[4].cpu().numpy()) == wantA
        tA[4].fill_(0x5a); torch.cuda.synchronize()
        a0, r0 = e.async_stats()
        run_dev(e, tA, nA, tag1, tA[4]); e.synchronize()
        assert bytes(tA[4].cpu().numpy()) == wantA and e.async_stats() == (a0 + 1, r0)     # enqueued on the guess of 40 keys
        held = hold_stream(torch, e, HOLD_MS)
        t_host = time.perf_counter()
        run_dev(e, tB, nB, tag1, tB[4])                                                   # pending; its guess fails (5000 > 1024)
        in_flight = 1
        if trigger == "five_in_flight":
            for bm in extra:
                run_dev(e, tA, nA, tag1, bm)
            in_flight = 4
        assert e.async_stats() == (a0 + 1 + in_flight, r0), "the calls ahead of C were not all enqueued asynchronously"
        t_host = 1e3 * (time.perf_counter() - t_host)
        assert not held.query(), "the hold of the stream ended before C was called: B may have been settled already"
        run_dev(e, tC, nC, tag2, tC[4])
        e.synchronize()
        gotC, gotB = bytes(tC[4].cpu().numpy()), bytes(tB[4].cpu().numpy())
        print("gpu_ctx_sequences A[%s-%s]: C popcount expected %d observed %d; host took %.2f ms from B to C"
              % (trigger, direction, popcount(wantC), popcount(gotC), t_host))
        assert gotC == wantC, "C (tag 2, %d tuples): popcount expected %d, observed %d" % (nC, popcount(wantC), popcount(gotC))
        assert gotB == wantB, "B (re-run): popcount expected %d, observed %d" % (popcount(wantB), popcount(gotB))
        assert e.async_stats()[1] == r0 + 1                                               # B was re-run, nothing else
        for bm in extra[:in_flight - 1]:
            assert bytes(bm.cpu().numpy()) == wantA
        tA[4].fill_(0x5a); torch.cuda.synchronize()
        run_dev(e, tA, nA, tag1, tA[4]); e.synchronize()
        assert bytes(tA[4].cpu().numpy()) == wantA
        sub = sample_of(nC, 5)                                                            # ... and the oracle on a sample of C under tag 2
        ob = oracle.verify_batch(b"".join(C[0][128 * i:128 * i + 128] for i in sub), [C[1][i] for i in sub],
                                 b"".join(C[2][64 * i:64 * i + 64] for i in sub), tag2, nthreads=4)
        assert [bit(ob, j) for j in range(len(sub))] == [bit(wantC, i) for i in sub]
    finally:
        e.close()


# ================================================================ B. the operation table

class Env:
    """what the operations are built from: the generator engine, the oracle, the module; caches of inputs and of device tensors"""
    def __init__(self, G, O, M, pyref):
        import torch
        self.G, self.O, self.M, self.pyref, self.torch = G, O, M, pyref, torch
        self.T = tags_of(M)
        self.cache = {}

    def batch(self, n, tag, pool, inv, key0=0):
        k = ("batch", n, tag, pool, inv, key0)
        if k not in self.cache:
            self.cache[k] = synth.make_batch_gpu(self.G, self.O, n, tag, pool=pool, invalid_every=inv, spot=4, key0=key0, seed=n + pool)
        return self.cache[k]

    def dev(self, n, tag, pool, inv, key0=0):
        k = ("dev", n, tag, pool, inv, key0)
        if k not in self.cache:
            b = self.batch(n, tag, pool, inv, key0)
            self.cache[k] = synth.dev_batch(self.M, self.torch, b[0], b[1], b[2])[:4]
        return self.cache[k]

    def points(self, n, seed):
        """P_i = [a_i] G1, Q_i = [b_i] G2 made by the generator engine, first and last checked against the oracle"""
        k = ("points", n, seed)
        if k not in self.cache:
            rnd = random.Random(seed)
            a = [rnd.randrange(1, R) for _ in range(n)]; b = [rnd.randrange(1, R) for _ in range(n)]
            G1, G2 = self.O.g1_generator(), self.O.g2_generator()
            P = self.G.g1_mul_batch(G1 * n, b"".join(map(b32, a)), n)
            Q = self.G.g2_mul_batch(G2 * n, b"".join(map(b32, b)), n)
            for i in (0, n - 1):
                assert P[64 * i:64 * i + 64] == self.O.g1_mul(G1, a[i]) and Q[128 * i:128 * i + 128] == self.O.g2_mul(G2, b[i])
            self.cache[k] = (a, b, P, Q)
        return self.cache[k]


class Op:
    """One entry of the table.  make(env) -> (run, check): run(engine) gives the operation's bytes on that engine (or, for a
    pending verify_batch_dev, a function that reads them later); check(bytes) compares them with the oracle / the closed form."""
    def __init__(self, family, n, tag, make, pending=False, product=False, label=""):
        self.family, self.n, self.tag, self.make, self.pending, self.product = family, n, tag, make, pending, product
        self.key = "%s/n=%d/tag=%s%s%s" % (family, n, tag, "/" + label if label else "", "/pending" if pending else "")
        self.built = None

    def build(self, env):
        if self.built is None:
            self.built = self.make(env)
        return self.built

    def describe(self, env):
        return "%s (n = %d, tag of %d bytes)" % (self.key, self.n, len(env.T[self.tag]))


def check_verify_bits(env, b, tag, out, seed=3):
    pks, msgs, sigs, exp = b
    n = len(msgs)
    want = synth.bitmap_of(exp)
    assert out == want, "bitmap differs from the closed form: popcount expected %d, observed %d" % (popcount(want), popcount(out))
    sub = sample_of(n, seed)
    ob = env.O.verify_batch(b"".join(pks[128 * i:128 * i + 128] for i in sub), [msgs[i] for i in sub],
                            b"".join(sigs[64 * i:64 * i + 64] for i in sub), tag, nthreads=4)
    assert [bit(ob, j) for j in range(len(sub))] == [bit(out, i) for i in sub], "bitmap differs from the oracle on the sample"


def op_verify(kind, n, tag, pool, inv=3, key0=0, pending=False):
    """kind: verify_batch / verify_batch_rlc (host pointers), verify_batch_dev / verify_batch_rlc_dev (device pointers)"""
    def make(env):
        tg = env.T[tag]
        b = env.batch(n, tg, pool, inv, key0)
        torch = env.torch

        def run(e):
            if kind == "verify_batch":
                return e.verify_batch(b[0], b[1], b[2], tg)
            if kind == "verify_batch_rlc":
                return e.verify_batch_rlc(b[0], b[1], b[2], tg)
            t = env.dev(n, tg, pool, inv, key0)
            bm = torch.full(((n + 7) // 8,), 0x5a, dtype=torch.uint8, device=t[0].device)      # one output buffer per call
            torch.cuda.synchronize()
            run_dev(e, t, n, tg, bm, rlc=kind == "verify_batch_rlc_dev")
            if pending:
                return lambda: bytes(bm.cpu().numpy())
            e.synchronize()
            return bytes(bm.cpu().numpy())
        return run, lambda out: check_verify_bits(env, b, tg, out)
    return Op(kind, n, tag, make, pending=pending, label="pool=%d/key0=%d" % (pool, key0))


def op_aggregate_verify(n, tag, pool):
    def make(env):
        tg = env.T[tag]
        pks, msgs, sigs, _ = env.batch(n, tg, pool, 0, 500)
        agg = env.O.aggregate_sigs(sigs, n)
        bad = list(msgs); bad[n // 2] = b"tampered"

        def run(e):
            return bytes([e.aggregate_verify(pks, msgs, agg, tg), e.aggregate_verify(pks, bad, agg, tg)])

        def check(out):
            assert out == b"\x01\x00"
            if n <= 300:
                assert env.O.aggregate_verify(pks, msgs, agg, tg) is True and env.O.aggregate_verify(pks, bad, agg, tg) is False
        return run, check
    return Op("aggregate_verify", n, tag, make, product=True, label="pool=%d" % pool)


def op_aggregate_partial_finish(n, tag):
    def make(env):
        tg = env.T[tag]
        pks, msgs, sigs, _ = env.batch(n, tg, n, 0, 700)
        agg = env.O.aggregate_sigs(sigs, n)
        k = n // 3 + 1

        def run(e):
            p0, ok0 = e.aggregate_partial(pks[:128 * k], msgs[:k], tg)
            p1, ok1 = e.aggregate_partial(pks[128 * k:], msgs[k:], tg)
            return p0 + p1 + bytes([ok0, ok1, e.aggregate_finish(p0 + p1, 2, agg), e.aggregate_finish(p0, 1, agg)])

        def check(out):
            assert out[768:] == b"\x01\x01\x01\x00"
            if n <= 300:
                h = env.O.hash_to_g1_batch(msgs, tg)
                assert out[:384] == env.O.multi_miller_loop(h[:64 * k], pks[:128 * k], k)
                assert out[384:768] == env.O.multi_miller_loop(h[64 * k:], pks[128 * k:], n - k)
        return run, check
    return Op("aggregate_partial_finish", n, tag, make, product=True)


def op_fast_aggregate_verify_batch(g, per, tag):
    def make(env):
        tg = env.T[tag]
        pool = 64
        sks = [synth.sk_of(3000 + k) for k in range(pool)]
        pk_pool = env.G.sk_to_pk_batch(b"".join(map(b32, sks)), pool)
        key_sets, msgs, agg_sk, exp = [], [], [], []
        for i in range(g):
            lo = (i * 37) % (pool - per)
            key_sets.append(pk_pool[128 * lo:128 * (lo + per)])
            agg_sk.append(sum(sks[lo:lo + per]) % R)
            msgs.append(synth.msg_of(50000 + i))
        sigs = env.G.sign_batch(b"".join(map(b32, agg_sk)), msgs, tg)      # [sum sk] H(msg) = the sum of the members' signatures
        for i in range(g):
            exp.append(i % 5 != 4)
            if not exp[i]:
                msgs[i] = bytes([msgs[i][0] ^ 1]) + msgs[i][1:]

        def check(out):
            assert out == synth.bitmap_of(exp)
            for i in sample_of(g, 7)[:18]:
                assert env.O.fast_aggregate_verify(key_sets[i], per, msgs[i], sigs[64 * i:64 * i + 64], tg) is exp[i]
        return (lambda e: e.fast_aggregate_verify_batch(key_sets, msgs, sigs, tg)), check
    return Op("fast_aggregate_verify_batch", g, tag, make, label="per=%d" % per)


def op_prepared(n, tag):
    """g2_prepare_batch + verify_batch_prepared + aggregate_verify_prepared on a table prepared by the engine under test"""
    def make(env):
        tg = env.T[tag]
        pool = min(5, n)
        b = env.batch(n, tg, pool, 4 if n > 1 else 0, 900)
        pks, msgs, sigs, exp = b
        keys = [env.O.sk_to_pk(synth.sk_of(900 + k)) for k in range(pool)] + [synth.NON_SUBGROUP_PK]
        idx = [keys.index(pks[128 * i:128 * i + 128]) for i in range(n)]
        good = [i for i in range(n) if exp[i]]
        agg = env.O.aggregate_sigs(b"".join(sigs[64 * i:64 * i + 64] for i in good), len(good))
        gm = [msgs[i] for i in good]; gi = [idx[i] for i in good]
        bad = list(gm); bad[-1] = b"tampered"

        def run(e):
            prep = e.g2_prepare_batch(b"".join(keys), len(keys))
            try:
                return (e.verify_batch_prepared(prep, idx, msgs, sigs, tg) + prep.valid_bitmap()
                        + bytes([e.aggregate_verify_prepared(prep, gi, gm, agg, tg), e.aggregate_verify_prepared(prep, gi, bad, agg, tg)]))
            finally:
                prep.close()

        def check(out):
            nb = (n + 7) // 8
            check_verify_bits(env, b, tg, out[:nb])
            assert out[nb:] == bytes([(1 << pool) - 1]) + b"\x01\x00"
            if len(good) <= 300:
                assert env.O.aggregate_verify(b"".join(keys[k] for k in gi), gm, agg, tg) is True
        return run, check
    return Op("prepared_keys", n, tag, make)


def op_pairing_batch(n):
    def make(env):
        a, b, P, Q = env.points(n, 11)

        def check(out):
            for i in sample_of(n, 2)[:18]:
                assert out[384 * i:384 * i + 384] == env.O.pairing_batch(P[64 * i:64 * i + 64], Q[128 * i:128 * i + 128], 1)
        return (lambda e: e.pairing_batch(P, Q, n)), check
    return Op("pairing_batch", n, "40", make)


def op_multi_miller_loop(n):
    def make(env):
        a, b, P, Q = env.points(n, 12)

        def check(out):
            assert n <= 300 and out == env.O.multi_miller_loop(P, Q, n)
        return (lambda e: e.multi_miller_loop(P, Q, n)), check
    return Op("multi_miller_loop", n, "40", make, product=True)


def equations(env, n_eq, lo, hi, seed):
    """ragged equations over closed-form points: equation g holds iff sum_j a_j b_j = 0 mod r; every third one is made to hold"""
    k = ("equations", n_eq, lo, hi, seed)
    if k not in env.cache:
        rnd = random.Random(seed)
        sizes = [rnd.randint(lo, hi) for _ in range(n_eq)]
        a, b, holds = [], [], []
        for g, sz in enumerate(sizes):
            ag = [rnd.randrange(1, R) for _ in range(sz)]; bg = [rnd.randrange(1, R) for _ in range(sz)]
            want = 0 if g % 3 == 0 else 1
            rest = sum(x * y for x, y in zip(ag[:-1], bg[:-1])) % R
            bg[-1] = (want - rest) * pow(ag[-1], -1, R) % R
            if bg[-1] == 0:
                bg[-1], want = 1, None                 # (never with random scalars; kept exact rather than assumed)
            holds.append(sum(x * y for x, y in zip(ag, bg)) % R == 0)
            a += ag; b += bg
        G1, G2 = env.O.g1_generator(), env.O.g2_generator()
        tot = len(a)
        P = env.G.g1_mul_batch(G1 * tot, b"".join(map(b32, a)), tot)
        Q = env.G.g2_mul_batch(G2 * tot, b"".join(map(b32, b)), tot)
        assert P[-64:] == env.O.g1_mul(G1, a[-1]) and Q[-128:] == env.O.g2_mul(G2, b[-1])
        env.cache[k] = (P, Q, np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64), holds)
    return env.cache[k]


def op_equations(family, n_eq, lo, hi):
    def make(env):
        P, Q, off, holds = equations(env, n_eq, lo, hi, 21)

        def oracle_ml(g):
            s, t = int(off[g]), int(off[g + 1])
            return env.O.multi_miller_loop(P[64 * s:64 * t], Q[128 * s:128 * t], t - s)

        def check(out):
            sub = sample_of(n_eq, 4)[:18]
            if family == "multi_miller_loop_batch":
                for g in sub:
                    assert out[384 * g:384 * g + 384] == oracle_ml(g)
            else:
                assert out == synth.bitmap_of(holds)
                for g in sub:
                    assert (env.O.final_exponentiation(oracle_ml(g), 1) == ONE_GT) == bool(bit(out, g))
        fn = (lambda e: e.multi_miller_loop_batch(P, Q, off)) if family == "multi_miller_loop_batch" else (lambda e: e.pairing_check_batch(P, Q, off))
        return fn, check
    return Op(family, n_eq, "40", make, product=True, label="pairs=%d..%d" % (lo, hi))


def op_msm(g2, n, window):
    """window: None leaves the context's setting alone (whatever an earlier call forced), 0 resets it to automatic, else forces it"""
    def make(env):
        a, b, P, Q = env.points(n, 13)
        rnd = random.Random(31 + n)
        ks = [rnd.randrange(R) for _ in range(n)]
        kb = b"".join(map(b32, ks))
        if g2:
            want = env.O.g2_mul(env.O.g2_generator(), sum(k * x for k, x in zip(ks, b)) % R)
        else:
            want = env.O.g1_mul(env.O.g1_generator(), sum(k * x for k, x in zip(ks, a)) % R)

        def run(e):
            if window is not None:
                e.set_msm_window(window)
            return e.g2_msm(Q, kb, n) if g2 else e.g1_msm(P, kb, n)

        def check(out):
            assert out == want
        return run, check
    return Op("g2_msm" if g2 else "g1_msm", n, "40", make, product=True, label="window=%s" % window)


def op_threshold(t):
    def make(env):
        rnd = random.Random(40 + t)
        coeffs = [rnd.randrange(1, R) for _ in range(t)]
        ids = rnd.sample(range(1, 4 * t + 1), t)

        def f(x):
            acc = 0
            for c in reversed(coeffs):
                acc = (acc * x + c) % R
            return acc
        tg = env.T["40"]
        h = env.O.hash_to_g1_batch([b"threshold message"], tg)
        parts = env.G.g1_mul_batch(h * t, b"".join(b32(f(i)) for i in ids), t)
        idb = b"".join(map(b32, ids))

        def check(out):
            assert out == env.O.sign(coeffs[0], b"threshold message", tg)
            if t <= 300:
                assert out == env.O.threshold_combine(idb, parts, t)
        return (lambda e: e.threshold_combine(idb, parts, t)), check
    return Op("threshold_combine", t, "40", make, product=True)


def op_aggregate_points(family, n):
    def make(env):
        pks, msgs, sigs, _ = env.batch(n, env.T["40"], max(2, n // 2), 0, 1100)
        if family == "aggregate_sigs":
            return (lambda e: e.aggregate_sigs(sigs, n)), (lambda out: _eq(out, env.O.aggregate_sigs(sigs, n)))
        return (lambda e: e.aggregate_pks(pks, n)), (lambda out: _eq(out, env.O.aggregate_pks(pks, n)))
    return Op(family, n, "40", make, product=True)


def _eq(a, b):
    assert a == b


def op_mul_batch(g2, n):
    def make(env):
        a, b, P, Q = env.points(n, 14)
        rnd = random.Random(50 + n)
        ks = [rnd.randrange(R) for _ in range(n)]
        kb = b"".join(map(b32, ks))

        def check(out):
            for i in sample_of(n, 6):
                if g2:
                    assert out[128 * i:128 * i + 128] == env.O.g2_mul(Q[128 * i:128 * i + 128], ks[i])
                else:
                    assert out[64 * i:64 * i + 64] == env.O.g1_mul(P[64 * i:64 * i + 64], ks[i])
        return ((lambda e: e.g2_mul_batch(Q, kb, n)) if g2 else (lambda e: e.g1_mul_batch(P, kb, n))), check
    return Op("g2_mul_batch" if g2 else "g1_mul_batch", n, "40", make)


def op_hash(family, n, tag):
    def make(env):
        tg = env.T[tag]
        rnd = random.Random(60 + n)
        msgs = [b"", b"abc"][:n] + [rnd.randbytes(rnd.randrange(0, 200)) for _ in range(max(0, n - 2))]

        def check(out):
            sub = sample_of(n, 8)
            sm = [msgs[i] for i in sub]
            if family == "hash_to_g1_batch":
                want = env.O.hash_to_g1_batch(sm, tg); sz = 64
            elif family == "hash_to_g2_batch":
                want = env.O.hash_to_g2_batch(sm, tg); sz = 128
            else:
                want = b"".join(b32(env.pyref.hash_to_scalar(m, tg)) for m in sm); sz = 32
            assert b"".join(out[sz * i:sz * i + sz] for i in sub) == want
        return (lambda e: getattr(e, family)(msgs, tg)), check
    return Op(family, n, tag, make)


def op_sign(n, tag):
    def make(env):
        tg = env.T[tag]
        sks = [synth.sk_of(1300 + k) for k in range(n)]
        msgs = [synth.msg_of(60000 + i) for i in range(n)]
        skb = b"".join(map(b32, sks))

        def check(out):
            for i in sample_of(n, 9):
                assert out[64 * i:64 * i + 64] == env.O.sign(sks[i], msgs[i], tg)
        return (lambda e: e.sign_batch(skb, msgs, tg)), check
    return Op("sign_batch", n, tag, make)


def op_pop(n, tag):
    """tag "40": the library's proof-of-possession tag (the default argument); another tag is passed explicitly"""
    def make(env):
        tg = env.M.POP_DST if tag == "40" else env.T[tag]
        sks = [synth.sk_of(1500 + k) for k in range(n)]
        skb = b"".join(map(b32, sks))
        pks = env.G.sk_to_pk_batch(skb, n)

        def run(e):
            proofs = e.pop_prove_batch(skb, n, tg)
            swapped = proofs[64:128] + proofs[:64] + proofs[128:] if n > 1 else proofs
            return proofs + e.pop_verify_batch(pks, proofs, n, tg) + e.pop_verify_batch(pks, swapped, n, tg)

        def check(out):
            nb = (n + 7) // 8
            for i in sample_of(n, 10):
                assert pks[128 * i:128 * i + 128] == env.O.sk_to_pk(sks[i])
                assert out[64 * i:64 * i + 64] == env.O.sign(sks[i], pks[128 * i:128 * i + 128], tg)
            assert out[64 * n:64 * n + nb] == synth.bitmap_of([True] * n)
            assert out[64 * n + nb:] == synth.bitmap_of(([False, False] if n > 1 else [True]) + [True] * max(0, n - 2))
        return run, check
    return Op("pop_prove_verify_batch", n, tag, make)


def op_field(op, per, n):
    def make(env):
        rng = np.random.default_rng(70 + op)
        def operand():
            x = rng.integers(0, 256, size=(n * per, 32), dtype=np.uint8)
            x[:, 0] %= 0x30                                             # below p
            return x.tobytes()
        a = operand()
        b = operand() if op in env.M.Engine.FIELD_OP_BINARY else None
        return (lambda e: e.field_op_batch(op, a, b, n)), (lambda out: _eq(out, env.O.field_op_batch(op, a, b, n)))
    return Op("field_op_batch", n, "40", make, label="op=%d" % op)


def op_gt_pow(n):
    def make(env):
        a, b, P, Q = env.points(7, 15)
        base = env.G.pairing_batch(P, Q, 7)
        assert base[:384] == env.O.pairing_batch(P[:64], Q[:128], 1)
        gt = (base * (n // 7 + 1))[:384 * n]
        rnd = random.Random(80 + n)
        ks = [rnd.randrange(R) for _ in range(n)]

        def check(out):
            for i in sample_of(n, 12)[:18]:
                assert out[384 * i:384 * i + 384] == env.O.gt_pow(gt[384 * i:384 * i + 384], ks[i])
        return (lambda e: e.gt_pow_batch(gt, b"".join(map(b32, ks)), n)), check
    return Op("gt_pow_batch", n, "40", make)


def build_table():
    """The operation table and the two fixed sequences.  A sequence is a list of (operation key, expectation); the expectation of
    a pending verify_batch_dev is "async" (enqueued on the guess, which holds) or "rerun" (enqueued on the guess, which fails: the
    call is re-run when the next entry point settles it), from the documented capacity rule; None where it is left open."""
    table = {}

    def reg(op):
        table.setdefault(op.key, op)
        return op.key

    def pend(n, tag, pool, key0=0):
        return reg(op_verify("verify_batch_dev", n, tag, pool, key0=key0, pending=True))

    def vbd(n, tag, pool, key0=0):
        return reg(op_verify("verify_batch_dev", n, tag, pool, key0=key0))
    V = lambda kind, n, tag, pool: reg(op_verify(kind, n, tag, pool))
    eqs = lambda fam, n_eq, lo, hi: reg(op_equations(fam, n_eq, lo, hi))
    big = 20000
    # -- sequence 1: sizes 1, 7, 1000, 4100, 20000 and back; a pending call in front of every other family; the capacity of the
    #    key tables is 1024 until a call with more keys has been settled, then the largest key count seen
    s1 = [
        (V("verify_batch", 1, "40", 1), None),
        (vbd(7, "0", 3), None),
        (reg(op_hash("hash_to_g1_batch", 7, "1")), None),
        (V("verify_batch_rlc", 1000, "1", 40), None),
        (vbd(1000, "40", 40), None),
        (pend(1000, "40b", 40, key0=100), "async"),            # same key count, other keys; tag of the same length, one byte changed
        (reg(op_aggregate_verify(7, "255", 3)), None),         # few keys; 7 pairs over the leftovers of 1000 tuples
        (pend(4100, "255", 4100), "rerun"),                    # every key distinct: 4100 > capacity 1024
        (reg(op_aggregate_verify(137, "256", 137)), None),     # all keys distinct
        (vbd(4100, "40", 40), None),
        (pend(1000, "1", 40), "async"),
        (reg(op_aggregate_partial_finish(21, "300")), None),
        (pend(big, "40", 9000), "rerun"),                      # more keys than the capacity (4100)
        (reg(op_fast_aggregate_verify_batch(1000, 4, "0")), None),
        (pend(big, "40b", 40), "async"),
        (reg(op_prepared(1000, "255b")), None),
        (pend(big, "0", big), "rerun"),                        # one lane per tuple, every key distinct: the re-run takes the exact path
        (reg(op_pairing_batch(7)), None),
        (vbd(4100, "40", 40), None),                           # (after an exact chunk the next call counts first)
        (pend(4100, "40", 40), "async"),
        (reg(op_multi_miller_loop(7)), None),
        (pend(1000, "40b", 40, key0=100), "async"),
        (eqs("multi_miller_loop_batch", 5, 1, 7), None),
        (pend(1000, "1", 40), "async"),
        (eqs("pairing_check_batch", 7, 1, 5), None),
        (pend(1000, "40", 40), "async"),
        (reg(op_msm(False, 7, 5)), None),                      # window forced to 5 ...
        (pend(1000, "40b", 40, key0=100), "async"),
        (reg(op_msm(True, 7, None)), None),                    # ... and still forced here
        (pend(1000, "1", 40), "async"),
        (reg(op_threshold(7)), None),
        (pend(1000, "40", 40), "async"),
        (reg(op_aggregate_points("aggregate_sigs", 7)), None),
        (pend(1000, "40b", 40, key0=100), "async"),
        (reg(op_aggregate_points("aggregate_pks", 7)), None),
        (pend(1000, "1", 40), "async"),
        (reg(op_mul_batch(False, 7)), None),
        (pend(1000, "40", 40), "async"),
        (reg(op_mul_batch(True, 7)), None),
        (pend(1000, "40b", 40, key0=100), "async"),
        (reg(op_hash("hash_to_g1_batch", 1000, "255b")), None),
        (pend(1000, "1", 40), "async"),
        (reg(op_hash("hash_to_g2_batch", 7, "256")), None),
        (pend(1000, "40", 40), "async"),
        (reg(op_hash("hash_to_scalar_batch", 7, "300")), None),
        (pend(1000, "40b", 40, key0=100), "async"),
        (reg(op_sign(7, "0")), None),
        (pend(1000, "1", 40), "async"),
        (reg(op_pop(7, "40")), None),
        (pend(1000, "40", 40), "async"),
        (reg(op_field(48, 12, 7)), None),
        (pend(1000, "40b", 40, key0=100), "async"),
        (reg(op_gt_pow(7)), None),
        (pend(1000, "1", 40), "async"),
        (V("verify_batch", 7, "300", 3), None),
        (pend(1000, "40", 40), "async"),
        (V("verify_batch_rlc", 7, "255", 3), None),
        (pend(1000, "40b", 40, key0=100), "async"),
        (V("verify_batch_rlc_dev", 7, "1", 3), None),
        (reg(op_msm(False, 7, 0)), None),                      # back to the automatic window
        (vbd(7, "1", 3), None),
        (V("verify_batch", 1, "40", 1), None),
    ]
    # -- sequence 2: starts large and comes down; five calls in a row, the first one failing its guess; larger product calls and
    #    the small ones right behind them; the MSM window changed between calls
    s2 = [
        (V("verify_batch", big, "300", 64), None),
        (V("verify_batch_rlc_dev", 4100, "256", 40), None),
        (vbd(4100, "255", 40), None),
        (pend(4100, "1", 4100), "rerun"),                      # capacity 1024 (64 keys seen at most): fails, and stays in the queue ...
        (pend(4100, "255b", 40, key0=100), "async"),
        (pend(1000, "40", 40), "async"),
        (pend(1000, "40b", 40, key0=100), "async"),
        (pend(1000, "255", 40), "async"),                      # ... the fifth call finds the queue full and names another tag
        (reg(op_threshold(300)), None),
        (reg(op_threshold(7)), None),
        (reg(op_aggregate_verify(1000, "40", 5)), None),
        (reg(op_aggregate_verify(7, "255", 3)), None),
        (pend(1000, "1", 40), "async"),
        (reg(op_msm(False, 1000, None)), None),
        (reg(op_msm(True, 137, 8)), None),
        (reg(op_msm(False, 7, None)), None),                   # window still forced to 8, 7 terms over the leftovers of 1000
        (reg(op_msm(True, 7, 0)), None),
        (eqs("pairing_check_batch", 1000, 2, 2), None),
        (eqs("pairing_check_batch", 7, 1, 5), None),
        (reg(op_multi_miller_loop(137)), None),
        (reg(op_multi_miller_loop(7)), None),
        (reg(op_pairing_batch(1000)), None),
        (pend(1000, "40", 40), "async"),
        (eqs("multi_miller_loop_batch", 5, 1, 7), None),
        (reg(op_gt_pow(1000)), None),
        (reg(op_field(3, 1, 1000)), None),
        (reg(op_fast_aggregate_verify_batch(7, 3, "1")), None),
        (reg(op_prepared(7, "40b")), None),
        (reg(op_pop(1000, "255")), None),
        (reg(op_sign(1000, "255b")), None),
        (reg(op_hash("hash_to_g2_batch", 1000, "1")), None),
        (reg(op_hash("hash_to_scalar_batch", 1000, "0")), None),
        (reg(op_mul_batch(False, 1000)), None),
        (reg(op_mul_batch(True, 1000)), None),
        (reg(op_aggregate_points("aggregate_sigs", 1000)), None),
        (reg(op_aggregate_points("aggregate_pks", 1000)), None),
        (reg(op_aggregate_points("aggregate_sigs", 7)), None),
        (reg(op_aggregate_points("aggregate_pks", 7)), None),
        (reg(op_aggregate_partial_finish(137, "40")), None),
        (reg(op_aggregate_partial_finish(21, "300")), None),
        (V("verify_batch_rlc", 4100, "40", 40), None),
        (V("verify_batch", 1, "0", 1), None),
    ]
    return table, s1, s2


def random_sequence(table, seed, length):
    """drawn over the sorted keys of the table: a change of the table reshuffles it.  Pending calls may follow each other (more
    than four fill the queue); their bitmaps are read after the next call that is not pending has returned."""
    rnd = random.Random(seed)
    keys = sorted(table)
    seq = [(rnd.choice(keys), None) for _ in range(length)]
    if table[seq[-1][0]].pending:
        seq.append((rnd.choice([k for k in keys if not table[k].pending]), None))
    return seq


_STATE = {}


def env_of(eng, oracle, M, pyref):
    if "env" not in _STATE:
        _STATE["env"] = Env(eng, oracle, M, pyref)
        _STATE["table"], _STATE["s1"], _STATE["s2"] = build_table()
        _STATE["fresh"] = {}
    return _STATE["env"]


def fresh_output(env, op):
    """the operation on a context of its own, checked against the oracle / the closed form; once per table entry"""
    fresh = _STATE["fresh"]
    if op.key not in fresh:
        run, check = op.build(env)
        e = env.M.Engine(0)
        try:
            out = run(e)
            if callable(out):
                e.synchronize()
                out = out()
        finally:
            e.close()
        try:
            check(out)
        except AssertionError as err:
            raise AssertionError("%s on a context of its own differs from the oracle: %s" % (op.describe(env), err))
        fresh[op.key] = out
    return fresh[op.key]


class Runner:
    """one long-lived context walking through a sequence, one step per call of step()"""
    def __init__(self, env, seq, name):
        self.env, self.seq, self.name = env, seq, name
        self.e = env.M.Engine(0)
        self.outs = [None] * len(seq)
        self.waiting = []          # (step, reader, expectation, async_stats before the call)
        self.i = 0

    def close(self):
        self.e.close()

    def where(self, i):
        table = _STATE["table"]
        prev = table[self.seq[i - 1][0]].describe(self.env) if i else "nothing (a new context)"
        return "%s step %d: %s, after %s" % (self.name, i, table[self.seq[i][0]].describe(self.env), prev)

    def settle(self):
        for j, read, _, _ in self.waiting:
            self.outs[j] = read()
        if self.waiting and all(w[2] for w in self.waiting):
            first, after = self.waiting[0][3], self.e.async_stats()
            want = sum(w[2] == "rerun" for w in self.waiting)
            assert after[1] - first[1] == want, "%s: %d of the pending calls were expected to be re-run, async_stats went %s -> %s" % (
                self.where(self.waiting[-1][0]), want, first, after)
        self.waiting = []

    def step(self):
        i = self.i
        key, expect = self.seq[i]
        op = _STATE["table"][key]
        run, _ = op.build(self.env)
        before = self.e.async_stats()
        try:
            out = run(self.e)
        except Exception as err:
            raise AssertionError("%s raised %r" % (self.where(i), err))
        if callable(out):
            if expect:
                assert self.e.async_stats()[0] == before[0] + 1, "%s: the call was not enqueued asynchronously (the sequence does not reach the queue)" % self.where(i)
            self.waiting.append((i, out, expect, before))
        else:
            self.outs[i] = out
            self.settle()          # the following call has returned: ENTER settled what was pending
        self.i += 1
        return self.i < len(self.seq)

    def finish(self):
        self.e.synchronize()
        self.settle()
        return self.outs


def compare(env, runner, outs):
    for i, (key, _) in enumerate(runner.seq):
        want = fresh_output(env, _STATE["table"][key])
        got = outs[i]
        if got != want:
            d = [j for j in range(min(len(got), len(want))) if got[j] != want[j]]
            raise AssertionError("%s: %d bytes on the long-lived context, %d on a context of its own; first difference at byte %s%s"
                                 % (runner.where(i), len(got), len(want), d[0] if d else "(length)",
                                    ", popcount %d against %d" % (popcount(got), popcount(want)) if "verify" in key else ""))


def run_alone(env, seq, name):
    r = Runner(env, seq, name)
    try:
        while r.step():
            pass
        outs = r.finish()
    finally:
        r.close()
    compare(env, r, outs)
    return outs


FAMILIES = {"verify_batch", "verify_batch_dev", "verify_batch_rlc", "verify_batch_rlc_dev", "aggregate_verify", "aggregate_partial_finish",
            "fast_aggregate_verify_batch", "prepared_keys", "pairing_batch", "multi_miller_loop", "multi_miller_loop_batch",
            "pairing_check_batch", "g1_msm", "g2_msm", "threshold_combine", "aggregate_sigs", "aggregate_pks", "g1_mul_batch", "g2_mul_batch",
            "hash_to_g1_batch", "hash_to_g2_batch", "hash_to_scalar_batch", "sign_batch", "pop_prove_verify_batch", "field_op_batch", "gt_pow_batch"}
PRODUCT = {"aggregate_verify", "aggregate_partial_finish", "multi_miller_loop", "multi_miller_loop_batch", "pairing_check_batch", "g1_msm", "g2_msm",
           "threshold_combine", "aggregate_sigs", "aggregate_pks"}


def test_the_fixed_sequences_cover_the_table(M):
    """Self-check of the sequences themselves (no GPU work): every family of the table is used, every family is at least once
    the call right behind a pending verify_batch_dev, one of those pending calls fails its guess, every product-type family runs
    at a small size that is not a power of two right behind a larger call, the sizes go up and down through the launch forms,
    the tag lengths cycle and two different tags of one length follow each other."""
    table, s1, s2 = build_table()
    T = tags_of(M)
    assert {op.family for op in table.values()} == FAMILIES
    used = {table[k].family for k, _ in s1 + s2}
    assert used == FAMILIES
    assert PRODUCT == {op.family for op in table.values() if op.product}
    behind, small_after_large, tag_pairs = set(), set(), set()
    failing_in_front = 0
    for seq in (s1, s2):
        ops = [table[k] for k, _ in seq]
        assert not ops[-1].pending
        for i in range(1, len(ops)):
            p, o = ops[i - 1], ops[i]
            if p.pending:
                if not o.pending:
                    behind.add(o.family)
                    failing_in_front += seq[i - 1][1] == "rerun"
            if o.product and o.n < 1000 and o.n & (o.n - 1) and p.n >= 1000:
                small_after_large.add(o.family)
            if T[p.tag] != T[o.tag] and len(T[p.tag]) == len(T[o.tag]):
                tag_pairs.add(len(T[p.tag]))
    assert behind == FAMILIES - {"verify_batch_dev"}, FAMILIES - behind
    assert failing_in_front >= 1
    assert small_after_large == PRODUCT, PRODUCT - small_after_large
    assert tag_pairs
    assert {len(T[table[k].tag]) for k, _ in s1} == {0, 1, 40, 255, 256, 300}
    sizes = [table[k].n for k, _ in s1 if table[k].family.startswith("verify_batch")]
    it = iter(sizes)
    assert all(any(x == w if w < 20000 else x >= w for x in it) for w in (1, 7, 1000, 4100, 20000, 7, 1)), sizes
    # the key sets of the asynchronous calls change in the three ways
    labels = [table[k].key for k, _ in s1 if table[k].pending]
    assert any("key0=100" in x for x in labels) and any("pool=9000" in x for x in labels) and any("pool=20000" in x for x in labels)


@pytest.mark.parametrize("which", ["fixed_1", "fixed_2", "seeded"])
def test_results_do_not_depend_on_the_history(eng, oracle, M, pyref, which):
    """Every operation of the sequence gives, on one long-lived context, the bytes it gives on a context of its own; those are
    checked against the oracle (everything up to 300 elements, the first, the last and 16 seeded elements beyond) and against
    the closed forms.  RLC verification draws its weights per call: its bitmap is what is compared."""
    env = env_of(eng, oracle, M, pyref)
    if which == "seeded":
        seq = random_sequence(_STATE["table"], 20261016, 45)
    else:
        seq = _STATE["s1"] if which == "fixed_1" else _STATE["s2"]
    outs = run_alone(env, seq, which)
    _STATE["alone_" + which] = outs


def test_two_contexts_on_one_gpu_interleaved(eng, oracle, M, pyref):
    """The first fixed sequence on two contexts, their calls interleaved step by step: each gives the bytes the sequence gives
    alone.  Contexts share only the device (the file-scope constant tables)."""
    env = env_of(eng, oracle, M, pyref)
    seq = _STATE["s1"]
    alone = _STATE.get("alone_fixed_1") or run_alone(env, seq, "fixed_1")
    ra, rb = Runner(env, seq, "interleaved a"), Runner(env, seq, "interleaved b")
    try:
        more = True
        while more:
            more = ra.step()
            assert rb.step() == more
        oa, ob = ra.finish(), rb.finish()
    finally:
        ra.close(); rb.close()
    for r, outs in ((ra, oa), (rb, ob)):
        compare(env, r, outs)
        for i in range(len(seq)):
            assert outs[i] == alone[i], "%s differs from the same step of the sequence run alone" % r.where(i)
