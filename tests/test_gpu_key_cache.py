"""GPU tests (MI355X) of the context's store of prepared keys (bls-bn254_amd/csrc/key_cache.h, k_keycache.hip): a key whose 128
bytes an earlier call on the context prepared is not prepared again, and nothing a call returns depends on that.

Every bitmap must equal the closed-form expectation of its batch AND, byte for byte, the bitmap of the same call sequence on a
second context whose store is switched off (set_key_cache(0)).  Batches have 1024 .. 4096 tuples over pools of 30 .. 40 keys;
a capacity of 64 keys is set where the store has to be emptied.  Expected values never come from the context under test."""
import pytest

from tests import synth
from tests.gpu_support import eng, M

pytestmark = pytest.mark.gpu


_BATCHES = {}


def batch(eng, oracle, M, name):
    """(pks, msgs, sigs, expected) by name, made once.  Every fifth signature is knocked off the curve, so every expected bitmap
    has both values in it; the keys of a batch are exactly its pool (make_batch_gpu's own corruptions would add keys)."""
    if name not in _BATCHES:
        n, pool, key0, base = {"A": (2048, 40, 0, 0), "A_new": (2048, 40, 0, 80000), "B": (2048, 30, 1000, 160000),
                               "A_small": (1024, 40, 0, 240000), "A_tri": (4096, 40, 0, 320000), "K": (4096, 1500, 3000, 400000)}[name]
        pks, msgs, sigs, exp = synth.make_batch_gpu(eng, oracle, n, M.DEFAULT_DST, pool=pool, invalid_every=0, spot=4, base=base, key0=key0)
        sigs = bytearray(sigs)
        for i in range(4, n, 5):
            sigs[64 * i + 63] ^= 1
            exp[i] = False
        _BATCHES[name] = (pks, msgs, bytes(sigs), exp)
    return _BATCHES[name]


def select(b, idx):
    pks, msgs, sigs, exp = b
    return (b"".join(pks[128 * i:128 * i + 128] for i in idx), [msgs[i] for i in idx], b"".join(sigs[64 * i:64 * i + 64] for i in idx),
            [exp[i] for i in idx])


def concat(a, b):
    return a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + b[3]


def distinct_keys(b):
    return len({b[0][128 * i:128 * i + 128] for i in range(len(b[1]))})


class Pair:
    """the context under test and its twin without a store: every call goes to both"""

    def __init__(self, M, torch, capacity=None):
        self.M, self.torch = M, torch
        self.on, self.off = M.Engine(0), M.Engine(0)
        self.off.set_key_cache(0)
        if capacity is not None:
            self.on.set_key_cache(capacity)
        self.dev = {}
        self.pending = []

    def close(self):
        self.on.close(); self.off.close()

    def tensors(self, key, b, which):
        if (key, which) not in self.dev:
            self.dev[(key, which)] = synth.dev_batch(self.M, self.torch, b[0], b[1], b[2])
        return self.dev[(key, which)]

    def enqueue(self, key, b, rlc=False, slot=0):
        """verify_batch_dev (or the RLC form) of batch b on both contexts, not synchronised; slot: a bitmap of its own per call in flight"""
        n = len(b[1])
        for which, e in (("on", self.on), ("off", self.off)):
            t = self.tensors((key, slot), b, which)
            t[4].fill_(0x5a)
            self.torch.cuda.synchronize()
            f = e.verify_batch_rlc_dev if rlc else e.verify_batch_dev
            f(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), n, t[4].data_ptr(), self.M.DEFAULT_DST)
        self.pending.append(((key, slot), b))

    def settle(self):
        self.on.synchronize(); self.off.synchronize()
        for key, b in self.pending:
            want = synth.bitmap_of(b[3])
            got_on, got_off = (bytes(self.tensors(key, b, w)[4].cpu().numpy()) for w in ("on", "off"))
            assert got_off == want, "%s: the context without a store differs from the expectation" % (key,)
            assert got_on == want, "%s: the context with the store differs from the expectation" % (key,)
            assert got_on == got_off
        self.pending = []

    def call(self, key, b, rlc=False):
        self.enqueue(key, b, rlc)
        self.settle()


@pytest.fixture()
def pair_of(M):
    import torch
    made = []

    def make(capacity=None):
        p = Pair(M, torch, capacity)
        made.append(p)
        return p
    yield make
    for p in made:
        p.close()


def test_repeat(eng, oracle, M, pair_of):
    A = batch(eng, oracle, M, "A")
    assert distinct_keys(A) == 40
    p = pair_of()
    assert p.on.key_cache_stats() == (0, 0, 0, 0) and p.off.key_cache_stats() == (0, 0, 0, 0)
    p.call("A", A)
    assert p.on.key_cache_stats() == (0, 40, 0, 40)
    p.call("A", A)
    assert p.on.key_cache_stats() == (40, 40, 0, 40)                          # the second call: 40 hits, no miss
    assert p.off.key_cache_stats() == (0, 0, 0, 0)
    assert p.on.path_stats() == p.off.path_stats() and p.on.async_stats() == p.off.async_stats() == (1, 0)


def test_reset(eng, oracle, M, pair_of):
    A, B = batch(eng, oracle, M, "A"), batch(eng, oracle, M, "B")
    assert distinct_keys(B) == 30
    # 14 of A's keys and 20 of B's: behind B's 30 resident keys they fit a store of 64 (30 + 34)
    mix = concat(select(A, [i for i in range(2048) if i % 40 < 14][:700]), select(B, [i for i in range(2048) if i % 30 < 20][:1300]))
    assert distinct_keys(mix) == 34 and 1024 <= len(mix[1]) <= 4096
    p = pair_of(capacity=64)
    # The first call counts its keys; the second is enqueued with the asynchronous path's capacity of 1024 keys, and making room
    # for that many empties the store once (a reallocation, not a reset).  From the third call on the store only changes on the device.
    p.call("A", A)
    assert p.on.key_cache_stats() == (0, 40, 0, 40)
    p.call("A", A)
    assert p.on.key_cache_stats() == (0, 80, 0, 40)
    # The begin kernel counts the batch's keys, not its misses (key_cache.h): 40 resident + 40 of the batch > 64 empties the store
    # although they are the same keys.  A key set stays resident up to half the capacity; 40 is more than 32.
    p.call("A", A)
    assert p.on.key_cache_stats() == (0, 120, 1, 40)
    p.call("B", B)                                                             # 40 + 30 > 64: emptied, then B's keys
    assert p.on.key_cache_stats() == (0, 150, 2, 30)
    p.call("mix", mix)                                                         # 30 + 34 = 64 fits: B's are resident, A's are not any more
    assert p.on.key_cache_stats() == (20, 164, 2, 44)
    p.call("B20", select(B, [i for i in range(2048) if i % 30 < 20][:1300]))   # 44 + 20 = 64 fits: all 20 resident
    assert p.on.key_cache_stats() == (40, 164, 2, 44)
    p.call("A", A)                                                             # 44 + 40 > 64
    assert p.on.key_cache_stats() == (40, 204, 3, 40)
    assert p.on.async_stats() == p.off.async_stats()


def test_invalid_keys_stay_invalid(eng, oracle, M, pair_of):
    pks, msgs, sigs, exp = batch(eng, oracle, M, "A")
    pks, exp = bytearray(pks), list(exp)
    off_curve = bytearray(pks[128 * 3:128 * 4]); off_curve[127] ^= 1
    for i in range(len(msgs)):
        if i % 40 == 3:
            pks[128 * i:128 * i + 128] = off_curve; exp[i] = False                       # not on the curve
        if i % 40 == 5:
            pks[128 * i:128 * i + 128] = synth.NON_SUBGROUP_PK; exp[i] = False           # on the curve, outside the subgroup
    bad = (bytes(pks), msgs, sigs, exp)
    assert distinct_keys(bad) == 40
    p = pair_of()
    p.call("bad", bad)
    assert p.on.key_cache_stats() == (0, 40, 0, 40)                           # both seen as misses first ...
    p.call("bad", bad)
    assert p.on.key_cache_stats() == (40, 40, 0, 40)                          # ... then as hits: their tuples are invalid both times
    p.call("bad", bad, rlc=True)
    assert p.on.key_cache_stats() == (80, 40, 0, 40)


def test_same_keys_new_data(eng, oracle, M, pair_of):
    A, A_new = batch(eng, oracle, M, "A"), batch(eng, oracle, M, "A_new")
    assert A[0] == A_new[0] and A[1] != A_new[1] and A[2] != A_new[2]
    p = pair_of()
    p.call("A", A)
    p.call("A_new", A_new)
    assert p.on.key_cache_stats() == (40, 40, 0, 40)
    p.call("A", A)
    assert p.on.key_cache_stats() == (80, 40, 0, 40)


def test_async_queue_of_four(eng, oracle, M, pair_of):
    A, B = batch(eng, oracle, M, "A"), batch(eng, oracle, M, "B")
    p = pair_of()
    p.call("A", A)                                                            # the first call counts; the next ones are enqueued on its key count
    a0 = p.on.async_stats()
    for slot, (key, b) in enumerate((("A", A), ("B", B), ("A", A), ("B", B))):
        p.enqueue(key, b, slot=slot)
    assert p.on.async_stats() == (a0[0] + 4, a0[1]) == p.off.async_stats()    # four in flight
    p.settle()
    assert p.on.async_stats() == (a0[0] + 4, a0[1]) == p.off.async_stats()    # none re-run
    assert p.on.key_cache_stats() == (40 + 40 + 30, 40 + 30, 0, 70)


def test_over_capacity_reruns_exactly_once(eng, oracle, M, pair_of):
    A, K = batch(eng, oracle, M, "A"), batch(eng, oracle, M, "K")
    assert distinct_keys(K) == 1500                                           # more than the 1024 keys the call is enqueued with
    p = pair_of()
    p.call("A", A)
    a0, r0 = p.on.async_stats()
    p.enqueue("K", K)
    assert p.on.async_stats() == (a0 + 1, r0)
    p.settle()
    assert p.on.async_stats() == (a0 + 1, r0 + 1) == p.off.async_stats()      # the existing re-run, once
    hits, misses, resets, resident = p.on.key_cache_stats()
    assert (resets, resident) == (0, 40 + 1500) and hits + misses == 40 + 1024 + 1500      # the discarded run looked 1024 keys up
    p.call("A", A)
    assert p.on.async_stats() == p.off.async_stats()
    assert p.on.key_cache_stats()[2:] == (0, 40 + 1500)


def test_small_and_tri_forms_use_the_store(eng, oracle, M, pair_of):
    small, tri = batch(eng, oracle, M, "A_small"), batch(eng, oracle, M, "A_tri")
    p = pair_of()
    for rep in range(2):
        p.call("small", small)                                                # n = 1024: one wave per tuple
        p.call("tri", tri)                                                    # n = 4096: three lanes per tuple
    assert p.on.key_cache_stats() == (120, 40, 0, 40)
    assert p.on.path_stats() == p.off.path_stats()


def test_two_contexts_have_stores_of_their_own(eng, oracle, M, pair_of):
    A, B = batch(eng, oracle, M, "A"), batch(eng, oracle, M, "B")
    p, q = pair_of(), pair_of()
    p.call("A", A); q.call("B", B)
    p.call("A", A); q.call("B", B)
    assert p.on.key_cache_stats() == (40, 40, 0, 40) and q.on.key_cache_stats() == (30, 30, 0, 30)
    q.call("A", A)                                                            # resident on the other context only
    assert q.on.key_cache_stats() == (30, 70, 0, 70) and p.on.key_cache_stats() == (40, 40, 0, 40)


def test_rlc_reuses_the_entries(eng, oracle, M, pair_of):
    A = batch(eng, oracle, M, "A")
    p = pair_of()
    p.call("A", A)
    assert p.on.key_cache_stats() == (0, 40, 0, 40)
    p.call("A", A, rlc=True)
    assert p.on.key_cache_stats() == (40, 40, 0, 40)                          # no miss
    p.call("A", A)
    assert p.on.key_cache_stats() == (80, 40, 0, 40)


# what a call on the context with the store launches beyond its twin, by profile name (key_cache.h; host_verify.hip prepare_keys,
# miller_ids, keys_valid): the lookup and the copy of the misses' tables, the tuples' store indices -- and on the RLC path the
# chunks' store indices as well, with the validity bytes gathered into batch key order
STORE_LAUNCHES = {"kd_cache_begin": 1, "kd_cache_clear": 1, "kd_cache_lookup": 1, "kd_cache_scatter": 1, "kd_cache_map": 1}
STORE_LAUNCHES_RLC = dict(STORE_LAUNCHES, kd_cache_map=2, kd_cache_ok=1)


@pytest.mark.parametrize("name,rlc,miller", [("A_small", False, "miller_wide_prepared"), ("A_tri", False, "miller_tri_prepared"), ("A", True, "miller_wide_prepared")])
def test_both_sources_of_tables_run_the_same_pipeline(eng, oracle, M, pair_of, name, rlc, miller):
    """The tables come from the store or from the call; everything else a call launches is the same.  Launch counts by name
    (profile_read) of the first call on a fresh context (it counts its keys; every key is new to the store) and of the second
    (enqueued on the first one's key count; every key resident): equal for every name of the twin, and the store's context has
    exactly the store's own launches besides.  In batch A every fifth signature is invalid: its RLC call fails the key round and
    runs the chunk round and the per-tuple fallback, so the store indices of keys, chunks and tuples are all used."""
    b = batch(eng, oracle, M, name)
    p = pair_of()
    for e in (p.on, p.off):
        e.profile_enable(True)
    for rep in range(2):
        for e in (p.on, p.off):
            e.profile_reset()
        p.call(name, b, rlc=rlc)                                              # settles: both contexts are synchronised
        on, off = ({k: v["launches"] for k, v in e.profile_read().items()} for e in (p.on, p.off))
        print(name, "call", rep, "with the store:", on, "twin:", off)
        assert off.get(miller, 0) >= 1 and "kd_propagate" in off and not any(k.startswith("kd_cache_") for k in off)
        assert {k: on.get(k) for k in off} == off
        assert {k: v for k, v in on.items() if k not in off} == (STORE_LAUNCHES_RLC if rlc else STORE_LAUNCHES)
    if not rlc:
        assert p.on.async_stats() == p.off.async_stats() == (1, 0)            # the second call took the asynchronous path
    assert p.on.key_cache_stats() == (40, 40, 0, 40)
