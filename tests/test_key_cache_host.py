"""CPU-only: the lane functions of the store of prepared keys (bls-bn254_amd/csrc/key_cache.h: begin / clear / lookup / end, the
code the kernels of k_keycache.hip run) driven by the stand-alone program tests/hostsim/key_cache_host.cpp over scripted
sequences of batches and compared, step by step, with a Python dict model.  The program is built twice -- plain, and with
-fsanitize=address,undefined -fno-sanitize-recover, every buffer exactly as large as the kernels' -- and both are run as
ordinary programs.  Capacity 8, slot table 16: collisions and wrap-around occur.  A test tool; the product has no CPU path."""
import random
import subprocess

import pytest

from tests import hostsim_build

C, M = 8, 16
U32 = 0xffffffff


def key_hash(pk, seed):
    """key_hash of key_cache.h"""
    h = (seed ^ 0x9e3779b9) & U32
    for k in range(32):
        h ^= int.from_bytes(pk[4 * k:4 * k + 4], "little")
        h = (h * 0x01000193) & U32
        h = ((h << 13) | (h >> 19)) & U32
    h ^= h >> 16; h = (h * 0x85ebca6b) & U32
    h ^= h >> 13; h = (h * 0xc2b2ae35) & U32
    h ^= h >> 16
    return h


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def prog(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("key_cache_" + request.param) / "key_cache_host"
    return hostsim_build.build("key_cache_host.cpp", exe, shared=False, extra=hostsim_build.SANITIZED if request.param == "sanitized" else ())


def keys_of(rnd, k):
    return [bytes(rnd.getrandbits(8) for _ in range(128)) for _ in range(k)]


def run(prog, tmp_path, seed, batches, cap=C, slots=M):
    """the program's steps: (reset, count, hits, misses, resets, slot_of, miss list, table, resident keys) per batch"""
    script = tmp_path / "script.txt"
    with open(script, "w") as f:
        f.write("%d %d %d\n" % (cap, slots, seed))
        for b in batches:
            f.write("B %d\n" % len(b))
            for k in b:
                f.write(k.hex() + "\n")
    out = subprocess.run([prog, str(script)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    steps, cur = [], None
    for line in out.stdout.splitlines():
        w = line.split()
        if w[0] == "batch":
            cur = {"reset": int(w[1]), "count": int(w[2]), "hits": int(w[3]), "misses": int(w[4]), "resets": int(w[5]), "keys": {}}
            steps.append(cur)
        elif w[0] == "slot_of":
            cur["slot_of"] = [int(x) for x in w[1:]]
        elif w[0] == "miss":
            cur["miss"] = [tuple(int(y) for y in x.split(":")) for x in w[1:]]
        elif w[0] == "table":
            cur["table"] = [int(x) for x in w[1:]]
        elif w[0] == "key":
            cur["keys"][int(w[1])] = bytes.fromhex(w[2])
    assert len(steps) == len(batches)
    return steps


def check(steps, batches, seed, cap=C, slots=M):
    """every step against the model: a dict key -> store index, emptied when it holds keys and count + batch > capacity"""
    model, hits, misses, resets = {}, 0, 0, 0
    for step, (s, b) in enumerate(zip(steps, batches)):
        assert len(set(b)) == len(b) <= cap
        reset = len(model) > 0 and len(model) + len(b) > cap
        if reset:
            model.clear(); resets += 1
        before = len(model)
        want_hit = [k in model for k in b]
        assert s["reset"] == int(reset), step
        new = []
        for j, k in enumerate(b):
            if want_hit[j]:
                assert s["slot_of"][j] == model[k], (step, j, "a resident key was not found at its place")
            else:
                new.append((j, s["slot_of"][j]))
        assert sorted(sl for _, sl in new) == list(range(before, before + len(new))), (step, "misses take the next store indices")
        assert sorted(s["miss"]) == sorted(new), (step, "the miss list names every miss with its place")
        for j, sl in new:
            model[b[j]] = sl
        hits += sum(want_hit); misses += len(new)
        assert (s["count"], s["hits"], s["misses"], s["resets"]) == (len(model), hits, misses, resets), step
        # the store holds exactly the model's keys, byte for byte: no stale entry survives a reset
        assert s["keys"] == {sl: k for k, sl in model.items()}, step
        # the slot table names every resident key once, and every key is reachable from its bucket without crossing a free slot
        taken = [x for x in s["table"] if x != -1]
        assert sorted(taken) == list(range(len(model))), step
        for k, sl in model.items():
            i = key_hash(k, seed) & (slots - 1)
            while s["table"][i] != sl:
                assert s["table"][i] != -1, (step, "a free slot lies between a key's bucket and its entry")
                i = (i + 1) & (slots - 1)


def both(prog, tmp_path, seed, batches):
    steps = run(prog, tmp_path, seed, batches)
    check(steps, batches, seed)
    return steps


def test_the_same_key_set_twice(prog, tmp_path):
    a = keys_of(random.Random(1), 4)
    s = both(prog, tmp_path, 77, [a, a, list(reversed(a))])
    assert (s[0]["hits"], s[0]["misses"]) == (0, 4)
    assert (s[1]["hits"], s[1]["misses"], s[1]["reset"]) == (4, 4, 0) and s[1]["miss"] == []         # the second pass is all hits
    assert (s[2]["hits"], s[2]["misses"]) == (8, 4) and s[2]["slot_of"] == list(reversed(s[0]["slot_of"]))


def test_append_at_capacity_and_reset_beyond_it(prog, tmp_path):
    k = keys_of(random.Random(2), 14)
    # count + batch = C: appended
    s = both(prog, tmp_path, 5, [k[:5], k[5:8]])
    assert [x["reset"] for x in s] == [0, 0] and s[1]["count"] == C
    # count + batch = C + 1: the store is emptied first; afterwards the first batch's keys are misses again, not stale hits
    s = both(prog, tmp_path, 5, [k[:5], k[5:9], k[:2], k[7:9]])
    assert [x["reset"] for x in s] == [0, 1, 0, 0] and [x["count"] for x in s] == [5, 4, 6, 6]
    assert len(s[2]["miss"]) == 2 and s[3]["miss"] == []
    assert all(s[2]["keys"][sl] == key for key, sl in zip(k[:2], s[2]["slot_of"]))
    # the rule counts the batch's keys, not its misses: a batch of hits that would not fit as misses empties the store too
    s = both(prog, tmp_path, 5, [k[:5], k[:4]])
    assert [x["reset"] for x in s] == [0, 1] and s[1]["count"] == 4


def test_keys_that_differ_in_the_last_four_bytes_only(prog, tmp_path):
    a = keys_of(random.Random(3), 1)[0]
    b = a[:124] + bytes(x ^ 0x80 for x in a[124:])
    c = a[:127] + bytes([a[127] ^ 1])
    s = both(prog, tmp_path, 9, [[a], [b], [a, b, c], [c, b, a]])
    assert [len(x["miss"]) for x in s] == [1, 1, 1, 0]
    assert len(set(s[3]["slot_of"])) == 3
    both(prog, tmp_path, 9, [[a, b, c], [c], [b], [a]])                       # ... arriving in one batch


def colliding(rnd, want_bucket=None):
    """two keys and a seed that puts both into one bucket of the 16-entry table (the given one, if any)"""
    a, b = keys_of(rnd, 2)
    for seed in range(1, 100000):
        ha, hb = key_hash(a, seed) & (M - 1), key_hash(b, seed) & (M - 1)
        if ha == hb and (want_bucket is None or ha == want_bucket):
            return a, b, seed
    raise AssertionError("no seed found")


def test_two_keys_in_one_bucket(prog, tmp_path):
    a, b, seed = colliding(random.Random(4))
    bucket = key_hash(a, seed) & (M - 1)
    assert bucket == key_hash(b, seed) & (M - 1)
    # b probes a's slot (filled by an earlier batch: compared in full, different) and takes the next one
    s = both(prog, tmp_path, seed, [[a], [b], [b, a]])
    assert s[1]["table"][bucket] == s[0]["slot_of"][0] and s[1]["table"][(bucket + 1) & (M - 1)] == s[1]["slot_of"][0]
    assert s[2]["miss"] == [] and s[2]["slot_of"] == [s[1]["slot_of"][0], s[0]["slot_of"][0]]
    # both in one batch: the second meets a slot claimed in the same pass and skips it unread
    s = both(prog, tmp_path, seed, [[a, b], [b], [a]])
    assert len(s[0]["miss"]) == 2 and s[1]["miss"] == [] and s[2]["miss"] == []


def test_a_batch_of_one_key(prog, tmp_path):
    a = keys_of(random.Random(5), 1)
    s = both(prog, tmp_path, 123, [a, a])
    assert (s[0]["count"], s[0]["slot_of"], s[0]["miss"]) == (1, [0], [(0, 0)]) and (s[1]["hits"], s[1]["misses"]) == (1, 1)


def test_a_batch_of_exactly_the_capacity_into_an_empty_store(prog, tmp_path):
    k = keys_of(random.Random(6), C + 2)
    s = both(prog, tmp_path, 31, [k[:C], k[C:C + 1], k[:C]])
    assert (s[0]["reset"], s[0]["count"], len(s[0]["miss"])) == (0, C, C)
    assert sum(x != -1 for x in s[0]["table"]) == C
    assert [x["reset"] for x in s[1:]] == [1, 1]                                # nothing fits behind a full store


def test_the_probe_wraps_past_the_last_slot(prog, tmp_path):
    a, b, seed = colliding(random.Random(7), want_bucket=M - 1)
    s = both(prog, tmp_path, seed, [[a], [b], [a, b]])
    assert s[1]["table"][M - 1] == s[0]["slot_of"][0] and s[1]["table"][0] == s[1]["slot_of"][0]        # b's entry is slot 0
    assert s[2]["miss"] == []
    s = both(prog, tmp_path, seed, [[b, a], [a, b]])
    assert s[0]["table"][M - 1] != -1 and s[0]["table"][0] != -1 and s[1]["miss"] == []


def test_scripted_random_sequences(prog, tmp_path):
    rnd = random.Random(8)
    pool = keys_of(rnd, 12)
    for seed in (1, 2, 3):
        batches = [rnd.sample(pool, rnd.randint(1, C)) for _ in range(40)]
        steps = both(prog, tmp_path, seed, batches)
        assert steps[-1]["resets"] > 0 and steps[-1]["hits"] > 0
