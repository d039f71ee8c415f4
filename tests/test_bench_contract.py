"""bench.py's launch contract (the parts that run without a GPU) and the shape of the bench line and rocprof summary
committed under profiles/ (fields and internal consistency only -- no performance numbers are asserted); on the GPU
(`-m gpu`), a plain run and a --full run at a reduced batch size."""
import csv
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEAN = ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "LOCAL_WORLD_SIZE", "GROUP_RANK")


def test_bench_rejects_world_size_mismatch():
    """WORLD_SIZE set by a launcher must equal --gpus: the check runs before anything touches the GPU."""
    env = {k: v for k, v in os.environ.items() if k not in CLEAN}
    env.update(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "WORLD_SIZE=1 but --gpus 2" in (out.stderr + out.stdout)


def test_bench_parent_spawns_n_ranks_and_relays_their_exit_code():
    """Plain `python bench.py --gpus 2` with WORLD_SIZE unset starts two ranks itself (torch.distributed.run).  Here there is
    no GPU, so both ranks must fail loudly at Engine creation (no CPU fallback) and the parent must relay the failure."""
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip("GPU present: covered by tests/test_gpu_sharded.py")
    env = {k: v for k, v in os.environ.items() if k not in CLEAN}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                          "--backend", "gloo", "--tuples-per-gpu", "64"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode != 0
    text = out.stderr + out.stdout
    assert "torch.distributed" in text or "ChildFailedError" in text or "rank" in text.lower()


def test_bench_options():
    """--full (the side measurements) and --dump-outputs DIR are parsed before anything touches the GPU"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "--full" in out.stdout and "--dump-outputs" in out.stdout


HEADLINE = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config")
SIDE = ("roofline", "kernel_ms", "algorithmic_fp_mul_per_verify", "exact_path", "rlc_path", "cpu_baseline")


def _bench_line(args):
    env = {k: v for k, v in os.environ.items() if k not in CLEAN}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args,
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_run_and_dump(tmp_path):
    """a plain run reports the headline only, and --dump-outputs writes the validity of every tuple of the last timed
    step (float32): the closed-form pattern of the synthetic batch, every 64th tuple invalid"""
    n = 32768
    j = _bench_line(["--steps", "3", "--warmup", "1", "--tuples-per-gpu", str(n), "--dump-outputs", str(tmp_path)])
    assert all(k in j for k in HEADLINE) and not any(k in j for k in SIDE)
    assert j["steps"] == 3 and j["warmup"] == 1 and j["value"] > 0 and j["ms_per_step"] > 0
    assert abs(n * 1e3 / j["ms_per_step"] / j["value"] - 1) < 0.01
    assert sorted(os.listdir(tmp_path)) == ["valid.npy"]
    v = np.load(str(tmp_path / "valid.npy"))
    assert v.dtype == np.float32 and v.shape == (n,)
    assert np.array_equal(v, np.array([0.0 if i % 64 == 63 else 1.0 for i in range(n)], dtype=np.float32))


@pytest.mark.gpu
def test_bench_full_run_keeps_the_side_measurements():
    """--full: per-kernel times, the roofline of the dominant kernel, the exact and RLC paths on the same batch and the
    CPU baseline beside the headline"""
    j = _bench_line(["--full", "--steps", "2", "--warmup", "1", "--tuples-per-gpu", "32768"])
    assert all(k in j for k in HEADLINE + SIDE)
    assert j["config"]["path"].startswith("prepared-keys") and j["roofline"]["kernel"] == "k_miller_prepared"
    assert j["roofline"]["achieved"] > 0 and j["exact_path"]["value"] > 0 and j["rlc_path"]["value"] > 0 and j["cpu_baseline"]["value"] > 0


def _latest(pattern):
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)))
    assert files, pattern
    return files[-1]


def test_committed_bench_line_has_the_contract_fields():
    b = json.load(open(_latest("r*_final_bench.json")))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in b, k
    assert b["unit"] == "verifies/s" and b["higher_is_better"] is True and b["vs_baseline"] is None
    assert "workload" in b["config"] and "model" not in b["config"]
    r = b["roofline"]
    assert r["bound"] == "valu" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    c = b["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and "sample" in c and "value" in c


def test_rocprof_summary_agrees_with_the_bench_line():
    """The dominant kernel's rocprofv3 average and the HIP-event figure behind roofline.achieved come from the same run
    class and must agree within a few percent; the work per launch is read from the line itself, not hard-coded."""
    bpath = _latest("r*_final_bench.json")
    tag = os.path.basename(bpath).split("_")[0]
    b = json.load(open(bpath))
    rows = {r["Name"].split("(")[0]: r for r in csv.DictReader(open(os.path.join(ROOT, "profiles", tag + "_final_kernel_stats.csv")))}
    avg_ms = float(rows[b["roofline"]["kernel"]]["AverageNs"]) / 1e6
    alg = b["algorithmic_fp_mul_per_verify"]
    per_tuple = alg.get("dominant_kernel") or (alg["miller_variable_pair"] + alg["miller_fixed_pair_lines"])
    mads = per_tuple * 136 * b["config"]["tuples_per_gpu"]
    assert abs(mads / (avg_ms * 1e-3) / 1e12 / b["roofline"]["achieved"] - 1) < 0.05
    if b["roofline"].get("traffic") is not None:
        t = json.load(open(os.path.join(ROOT, "profiles", tag + "_traffic.json")))
        assert t["kernels"][b["roofline"]["kernel"]]["hbm_bytes_per_launch"] == b["roofline"]["traffic"]


def test_scripts_compile():
    """every helper script under scripts/ (GPU benchmarks, profiling summaries, differential runs) at least parses"""
    import py_compile
    d = os.path.join(ROOT, "scripts")
    for f in sorted(os.listdir(d)):
        if f.endswith(".py"):
            py_compile.compile(os.path.join(d, f), doraise=True)


def test_executed_mads_and_rank_fields_of_the_committed_lines():
    """roofline.executed_mads_per_tuple is the hostsim count committed beside it (scripts/executed_mads.py), priced consistently;
    the committed N > 1 rehearsal line carries the per-rank spread and the all-reduce time."""
    b = json.load(open(_latest("r*_final_bench.json")))
    r = b["roofline"]
    if r.get("executed_mads_per_tuple") is not None:
        e = json.load(open(os.path.join(ROOT, "profiles", "r03_executed_mads.json")))
        ph = [v for k, v in e["phases"].items() if "(" + r["kernel"] + ")" in k]
        assert len(ph) == 1 and ph[0]["executed_mads"] == r["executed_mads_per_tuple"]
        m = e["mads_per_op"]
        assert ph[0]["executed_mads"] == (m["fp_mul"] * ph[0]["fp_mul"] + m["fp_sqr"] * ph[0]["fp_sqr"] + m["fp_dot2"] * ph[0]["fp_dot2"]
                                          + m["fp_lc_term"] * ph[0]["fp_lc_terms"])
        assert abs(r["achieved_executed"] / r["achieved"] - r["executed_over_algorithmic"]) < 0.01
    n2 = glob.glob(os.path.join(ROOT, "profiles", "r03_n2_rehearsal_one_gpu.json"))
    if n2:
        j = json.loads(open(n2[0]).read().strip().splitlines()[-1])
        assert j["n_gpus"] == 2 and j["scaling"] == "weak" and "cpu_baseline" not in j
        for k in ("ms_per_step_min", "ms_per_step_max", "allreduce_ms_min", "allreduce_ms_max", "datagen_s_max"):
            assert k in j["ranks"], k
        assert j["ranks"]["ms_per_step_min"] <= j["ranks"]["ms_per_step_max"] <= j["ms_per_step"] * 1.01
