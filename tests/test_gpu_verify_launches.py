"""The launches of the verify path and of the primitives under it (host.hip, host_verify.hip, the aggregate verify of
host_aggregate.hip), scenario by scenario: how often every kernel is launched (the engine's launch record, profile_read) and
what path_stats, async_stats, aggregate_path_stats and key_cache_stats move by, compared with tests/golden/verify_launches.json.
That file was recorded by this module against the library of the commit BEFORE the launch-form rule moved into launch_forms.h
and the verify path's state into workspaces (BLSBN254_LIB=<that build> python -m tests.test_gpu_verify_launches), so the
comparison says that every call still makes the launches it made.  Every scenario's result is also compared with its closed
form or the oracle.  Each scenario runs on an engine of its own: the key-count hint and the store of prepared keys are state.

The inputs are one table of 16 oracle-signed tuples over 4 keys, tiled: tuple i is entry i mod 16 under key i mod 4, and entry 5
carries entry 9's signature (the same key, another message: a point of the group, and wrong)."""
import json
import os

import numpy as np
import pytest

from tests import gpu_support, synth
from tests.gpu_support import M  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "verify_launches.json")
KNOBS = gpu_support.MILLER_FORM_KNOBS + ("BLSBN254_KEY_CACHE",)
SCENARIOS = ("verify_wide", "verify_tri", "verify_lane", "verify_no_store", "verify_exact", "verify_chunked", "verify_prepared", "pairing_wide", "pairing_tri",
             "miller_lane", "final_exp_split", "aggregate_repeated_keys", "aggregate_distinct_keys", "verify_dev_async_rerun")
STATS = ("path_stats", "async_stats", "aggregate_path_stats", "key_cache_stats")
ASYNC_KEYS = 1100           # more than the 1024 keys the asynchronous call is enqueued with


class Table:
    def __init__(self, oracle, dst):
        self.dst = dst
        self.sks = [synth.sk_of(70 + k) for k in range(4)]
        self.pks = [oracle.sk_to_pk(s) for s in self.sks]
        self.msgs = [synth.msg_of(7000 + j) for j in range(16)]
        self.good = [oracle.sign(self.sks[j % 4], self.msgs[j], dst) for j in range(16)]
        self.sigs = list(self.good)
        self.sigs[5] = self.good[9]
        self.g1, self.g2 = oracle.g1_generator(), oracle.g2_generator()
        self.ml = oracle.miller_loop_batch(self.g1, self.g2, 1)
        self.gt = oracle.pairing_batch(self.g1, self.g2, 1)
        # 40 pairs under 40 keys of their own, and their aggregate signature
        self.sks40 = [synth.sk_of(200 + k) for k in range(40)]
        self.pks40 = b"".join(oracle.sk_to_pk(s) for s in self.sks40)
        self.msgs40 = [synth.msg_of(7100 + k) for k in range(40)]
        self.agg40 = oracle.aggregate_sigs(b"".join(oracle.sign(s, m, dst) for s, m in zip(self.sks40, self.msgs40)), 40)
        self.oracle = oracle

    def batch(self, n):
        return b"".join(self.pks[i % 4] for i in range(n)), [self.msgs[i % 16] for i in range(n)], b"".join(self.sigs[i % 16] for i in range(n))

    def bits(self, n):
        return synth.bitmap_of([i % 16 != 5 for i in range(n)])

    def aggregate(self, n):
        """n pairs of the table with the valid signatures, and their sum"""
        pks, msgs, _ = self.batch(n)
        return pks, msgs, self.oracle.aggregate_sigs(b"".join(self.good[i % 16] for i in range(n)), n)


@pytest.fixture(scope="module")
def table(oracle, M):
    return Table(oracle, M.DEFAULT_DST)


def cus_of():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def verify_dev_async_rerun(M, e, T):
    """verify_batch_dev twice on one context: 64 tuples over the 4 keys (the counting path; leaves the hint), then 2049 tuples
    whose first ASYNC_KEYS carry keys of their own -- enqueued for 1024 keys without a read-back, so the check fails and
    synchronize() re-runs the batch.  Those tuples' signatures are the table's, under other keys: their bits are 0."""
    import torch
    n = 2049
    pks, msgs, sigs = T.batch(n)
    own = e.sk_to_pk_batch(b"".join(synth.sk_of(5000 + k).to_bytes(32, "big") for k in range(ASYNC_KEYS)), ASYNC_KEYS)
    pks = own + pks[128 * ASYNC_KEYS:]
    first, second = synth.dev_batch(M, torch, *T.batch(64)), synth.dev_batch(M, torch, pks, msgs, sigs)
    s0 = {k: getattr(e, k)() for k in STATS}
    e.profile_enable(True); e.profile_reset()
    for t, m in ((first, 64), (second, n)):
        e.verify_batch_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), m, t[4].data_ptr(), T.dst)
    e.synchronize()
    got = (bytes(first[4].cpu().numpy()), bytes(second[4].cpu().numpy()))
    want = (T.bits(64), synth.bitmap_of([i >= ASYNC_KEYS and i % 16 != 5 for i in range(n)]))
    return s0, got, want


def run_scenario(M, mp, T, name, cus):
    """-> {"launches": {kernel: count}, "stats": {getter: its counters' increase}}, the call's result, the expected one"""
    chunk, knobs, setup = None, None, lambda e: None
    if name.startswith("verify_") and name not in ("verify_prepared", "verify_dev_async_rerun"):
        n = {"verify_wide": 64, "verify_tri": 2049, "verify_lane": cus * 64 + 1, "verify_no_store": 2049, "verify_exact": 65, "verify_chunked": 209}[name]
        chunk = "64" if name == "verify_chunked" else None
        if name == "verify_no_store":
            setup = lambda e: e.set_key_cache(0)
        if name == "verify_exact":
            setup = lambda e: e.set_auto_prepare(False)
        call, want = (lambda e: e.verify_batch(*T.batch(n), T.dst)), T.bits(n)
    elif name == "verify_prepared":
        pks, msgs, sigs = T.batch(65)
        call, want = (lambda e: e.verify_batch_prepared(e.g2_prepare_batch(b"".join(T.pks), 4), np.arange(65, dtype=np.uint32) % 4, msgs, sigs, T.dst)), T.bits(65)
    elif name in ("pairing_wide", "pairing_tri"):
        n = 1 if name == "pairing_wide" else 1025
        call, want = (lambda e: e.pairing_batch(T.g1 * n, T.g2 * n, n)), T.gt * n
    elif name == "miller_lane":
        knobs = {"BLSBN254_WIDE_FE": "0", "BLSBN254_TRI_MAX": "0"}
        call, want = (lambda e: e.miller_loop_batch(T.g1 * 65, T.g2 * 65, 65)), T.ml * 65
    elif name == "final_exp_split":
        n = cus * 128
        call, want = (lambda e: e.final_exponentiation(T.ml * n, n)), T.gt * n
    elif name == "aggregate_repeated_keys":
        args = T.aggregate(1100)
        call, want = (lambda e: e.aggregate_verify(*args, T.dst)), True
    elif name == "aggregate_distinct_keys":
        call, want = (lambda e: e.aggregate_verify(T.pks40, T.msgs40, T.agg40, T.dst)), True
    e = gpu_support.fresh_engine(M, mp, chunk, knobs)
    try:
        setup(e)
        if name == "verify_dev_async_rerun":
            s0, got, want = verify_dev_async_rerun(M, e, T)
        else:
            s0 = {k: getattr(e, k)() for k in STATS}
            e.profile_enable(True); e.profile_reset()
            got = call(e)
        rec = e.profile_read()
        e.profile_enable(False)
        s1 = {k: getattr(e, k)() for k in STATS}
    finally:
        e.close()
    stats = {k: [b - a for a, b in zip(s0[k], s1[k])] for k in STATS}
    return {"launches": {k: v["launches"] for k, v in sorted(rec.items())}, "stats": stats}, got, want


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENARIOS)
def test_launches_are_the_recorded_ones(M, table, monkeypatch, name):
    if any(k in os.environ for k in KNOBS):
        pytest.skip("the environment sets %s: not the settings the record was made under" % ", ".join(k for k in KNOBS if k in os.environ))
    with open(GOLDEN) as f:
        golden = json.load(f)
    rec, got, want = run_scenario(M, monkeypatch, table, name, cus_of())
    assert got == want
    print(name, json.dumps(rec))
    assert rec["launches"] == golden[name]["launches"]
    assert rec["stats"] == golden[name]["stats"]


def test_what_the_scenarios_are_about():
    """the record itself shows the forms and paths the scenarios are named after"""
    with open(GOLDEN) as f:
        g = json.load(f)
    L = {k: v["launches"] for k, v in g.items()}
    for name, miller, hard in (("verify_wide", "miller_wide_prepared", "fe_hard_wide"), ("verify_tri", "miller_tri_prepared", "fe_tri_hard"),
                               ("verify_lane", "miller_prepared", "fe_h3"), ("verify_prepared", "miller_wide_prepared", "fe_hard_wide")):
        assert L[name][miller] == 1 and L[name][hard] == 1 and g[name]["stats"]["path_stats"] == [0 if name == "verify_prepared" else 1, 0], name
    assert "kd_cache_lookup" in L["verify_tri"] and "kd_cache_lookup" not in L["verify_no_store"] and L["verify_no_store"]["miller_tri_prepared"] == 1
    assert L["verify_exact"]["miller_verify"] == 1 and g["verify_exact"]["stats"]["path_stats"] == [0, 1]
    assert L["verify_chunked"]["miller_wide_prepared"] == 4 and g["verify_chunked"]["stats"]["path_stats"] == [4, 0]          # 64 + 64 + 64 + 17
    assert L["pairing_wide"]["miller_wide_1"] == 1 and L["pairing_tri"]["miller_tri_1"] == 1 and L["miller_lane"]["miller_1"] == 1
    assert all(L["final_exp_split"][k] == 1 for k in ("fe_easy_head", "fe_inv4", "fe_easy_tail")) and "fe_easy" not in L["final_exp_split"]
    assert g["aggregate_repeated_keys"]["stats"]["aggregate_path_stats"] == [1, 0] and L["aggregate_repeated_keys"]["miller_wide_1p"] == 1      # 4 keys + the signature's pair
    assert g["aggregate_distinct_keys"]["stats"]["aggregate_path_stats"] == [1, 0] and L["aggregate_distinct_keys"]["miller_wide_1p"] == 1
    s = g["verify_dev_async_rerun"]["stats"]
    assert s["async_stats"] == [1, 1] and s["path_stats"] == [2, 0]          # one call enqueued on the hint, and re-run


if __name__ == "__main__":
    # the recorder: every scenario against the library BLSBN254_LIB names (or the built one), written to the path given
    import sys
    import blsbn254_loader
    from oracle import oracle as O
    O.build()
    mod = blsbn254_loader.load()
    T, mp, out = Table(O, mod.DEFAULT_DST), pytest.MonkeyPatch(), {}
    for nm in SCENARIOS:
        out[nm], got, want = run_scenario(mod, mp, T, nm, cus_of())
        assert got == want, nm
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
