"""The launches of the batch verification by random linear combination (host_rlc.hip), scenario by scenario: how often every
kernel is launched (the engine's launch record, profile_read) and what the six counters of rlc_stats move by, compared with
tests/golden/rlc_launches.json.  That file was recorded by this module against the library of the commit BEFORE the host side was
split into workspaces, a plan header and one function per round (BLSBN254_LIB=<that build> python -m tests.test_gpu_rlc_launches),
so the comparison says that every call still makes the launches it made.  Every scenario's bitmap is also compared with
verify_batch's.  Each scenario runs on an engine of its own: the back-off and the store of prepared keys are state."""
import json
import os

import pytest

from tests import gpu_support, synth
from tests.gpu_support import M  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rlc_launches.json")
SEED = bytes(range(32))
KNOBS = gpu_support.MILLER_FORM_KNOBS + ("BLSBN254_RLC_GROUP", "BLSBN254_RLC_KEY_ROUND", "BLSBN254_KEY_CACHE")
SCENARIOS = ("key_round_passes", "key_round_fails", "key_round_off", "two_levels_of_key_sums", "distinct_keys", "chunked_entry", "no_key_store")


class Batches:
    """209 tuples, tuple i under key i mod 4; 200 under key i mod 2; 15 under key i mod 8.  swapped(): tuple 5's signature
    replaced by tuple 9's (the same key, another message: a point of the group, and wrong)"""

    def __init__(self, oracle, dst):
        self.dst = dst
        self.sks = [synth.sk_of(40 + k) for k in range(8)]
        self.pkp = [oracle.sk_to_pk(s) for s in self.sks]
        self.msgs = [synth.msg_of(9000 + i) for i in range(209)]
        self.sig = {}
        for pool, n in ((4, 209), (2, 200), (8, 15)):
            for i in range(n):
                if (i % pool, i) not in self.sig:
                    self.sig[(i % pool, i)] = oracle.sign(self.sks[i % pool], self.msgs[i], dst)

    def batch(self, n, pool, swapped=False):
        sigs = [self.sig[(i % pool, i)] for i in range(n)]
        if swapped:
            sigs[5] = sigs[9]
        return b"".join(self.pkp[i % pool] for i in range(n)), self.msgs[:n], b"".join(sigs)


@pytest.fixture(scope="module")
def batches(oracle, M):
    return Batches(oracle, M.DEFAULT_DST)


def run_scenario(M, mp, B, name):
    """-> {"launches": {kernel: count}, "stats": the six counters' increase, in rlc_stats' order}, the RLC bitmap, verify_batch's
    (made after the record: the RLC call meets an empty store of prepared keys)"""
    chunk, group, key_round, key_cache = None, 0, True, None
    if name in ("key_round_passes", "no_key_store"):
        args = B.batch(96, 4)                                           # the key round decides
        key_cache = 0 if name == "no_key_store" else None
    elif name in ("key_round_fails", "key_round_off"):
        args = B.batch(96, 4, swapped=True)                             # key 1 fails, its 2 chunks are checked, one goes to the fallback
        key_round = name == "key_round_fails"
    elif name == "two_levels_of_key_sums":
        args, group = B.batch(200, 2), 2                                # 50 chunks per key: more than key_sums sums in one level
    elif name == "distinct_keys":
        args = B.batch(15, 8, swapped=True)                             # 2 u > n: groups of 16 in the caller's order, the group fails
    elif name == "chunked_entry":
        args, chunk = B.batch(209, 4, swapped=True), "64"               # 64 + 64 + 64 + 17: a failed key round, two skipped, one passed
    e = gpu_support.fresh_engine(M, mp, chunk)
    try:
        if key_cache is not None:
            e.set_key_cache(key_cache)
        if group:
            e.set_rlc_group(group)
        if not key_round:
            e.set_rlc_key_round(False)
        s0 = e.rlc_stats()
        e.profile_enable(True); e.profile_reset()
        got = e.verify_batch_rlc(*args, B.dst, seed=SEED)
        rec = e.profile_read()
        e.profile_enable(False)
        s1 = e.rlc_stats()
        want = e.verify_batch(*args, B.dst)
    finally:
        e.close()
    return {"launches": {k: v["launches"] for k, v in sorted(rec.items())}, "stats": [s1[k] - s0[k] for k in s0]}, got, want


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENARIOS)
def test_launches_are_the_recorded_ones(M, batches, monkeypatch, name):
    if any(k in os.environ for k in KNOBS):
        pytest.skip("the environment sets %s: not the settings the record was made under" % ", ".join(k for k in KNOBS if k in os.environ))
    with open(GOLDEN) as f:
        golden = json.load(f)
    rec, got, want = run_scenario(M, monkeypatch, batches, name)
    assert got == want
    n = {"two_levels_of_key_sums": 200, "distinct_keys": 15, "chunked_entry": 209}.get(name, 96)
    valid = name in ("key_round_passes", "two_levels_of_key_sums", "no_key_store")
    assert want == synth.bitmap_of([valid or i != 5 for i in range(n)])            # tuple 5 carries the swapped signature
    print(name, json.dumps(rec))
    assert rec["launches"] == golden[name]["launches"]
    assert rec["stats"] == golden[name]["stats"]


def test_what_the_scenarios_are_about():
    """the record itself shows the paths the scenarios are named after"""
    with open(GOLDEN) as f:
        g = json.load(f)
    tuples, chunks, fallback, distinct, rounds, passed = range(6)
    assert g["key_round_passes"]["stats"] == [96, 0, 0, 0, 1, 1] and "rlc2_valid_fast" in g["key_round_passes"]["launches"]
    s = g["key_round_fails"]["stats"]
    assert (s[tuples], s[chunks], s[rounds], s[passed]) == (96, 2, 1, 0) and 0 < s[fallback] <= 16
    s = g["key_round_off"]["stats"]
    assert (s[tuples], s[chunks], s[rounds]) == (96, 8, 0) and "rlc2_keys_pass" not in g["key_round_off"]["launches"]
    assert g["two_levels_of_key_sums"]["launches"]["g1_seg_sum"] == 4           # two point arrays, two levels
    assert g["distinct_keys"]["stats"][distinct] == 15 and g["distinct_keys"]["launches"]["miller_verify"] == 1
    s = g["chunked_entry"]["stats"]
    assert (s[tuples], s[rounds], s[passed]) == (209, 2, 1)
    assert g["no_key_store"]["stats"] == g["key_round_passes"]["stats"] and g["no_key_store"]["launches"] != g["key_round_passes"]["launches"]


if __name__ == "__main__":
    # the recorder: every scenario against the library BLSBN254_LIB names (or the built one), written to the path given
    import sys
    import blsbn254_loader
    from oracle import oracle as O
    O.build()
    mod = blsbn254_loader.load()
    B, mp, out = Batches(O, mod.DEFAULT_DST), pytest.MonkeyPatch(), {}
    for nm in SCENARIOS:
        out[nm], got, want = run_scenario(mod, mp, B, nm)
        assert got == want, nm
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
