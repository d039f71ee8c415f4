"""CPU-only: the multi-scalar multiplication kernels exist in the built library, and the bucket accumulation and reduction
kernels keep every value in registers (0 bytes of scratch per lane)."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
MSM_KERNELS = ("k_msm_g1_prep", "k_msm_g2_prep", "k_kd_msm_hist", "k_kd_msm_scatter", "k_msm_g1_bucket", "k_msm_g2_bucket",
               "k_msm_g1_reduce", "k_msm_g2_reduce", "k_msm_g1_final", "k_msm_g2_final")
ZERO_SCRATCH = ("k_msm_g1_bucket", "k_msm_g2_bucket", "k_msm_g1_reduce", "k_msm_g2_reduce")


def _scratch():
    import blsbn254_loader
    M = blsbn254_loader.load()
    path = M.library_path()
    if not os.path.exists(path):
        __import__("bls_bn254_amd.build", fromlist=["x"]).build()
    from kernel_resources import code_objects
    tmp = tempfile.mkdtemp()
    out = {}
    for idx, (data, off, size) in enumerate(code_objects(path)):
        co = os.path.join(tmp, "co_%d.o" % idx)
        open(co, "wb").write(data[off:off + size])
        notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s*(\S+)", blk).group(1)
            if name.startswith("_Z"):
                name = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.split("(")[0].strip()
            out[name] = int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk).group(1))
    return out


def test_msm_kernels_built_and_accumulation_without_scratch():
    scratch = _scratch()
    missing = [k for k in MSM_KERNELS if k not in scratch]
    assert not missing, missing
    bad = {k: scratch[k] for k in ZERO_SCRATCH if scratch[k] != 0}
    assert not bad, "scratch bytes per lane in the bucket accumulation / reduction kernels: %s" % bad
