"""CPU-only: the multi-scalar multiplication kernels exist in the built library, and the bucket accumulation and reduction
kernels keep every value in registers (0 bytes of scratch per lane)."""
from tests.library_support import scratch_bytes

MSM_KERNELS = ("k_msm_g1_prep", "k_msm_g2_prep", "k_kd_msm_hist", "k_kd_msm_scatter", "k_msm_g1_bucket", "k_msm_g2_bucket",
               "k_msm_g1_reduce", "k_msm_g2_reduce", "k_msm_g1_final", "k_msm_g2_final")
ZERO_SCRATCH = ("k_msm_g1_bucket", "k_msm_g2_bucket", "k_msm_g1_reduce", "k_msm_g2_reduce")


def test_msm_kernels_built_and_accumulation_without_scratch():
    scratch = scratch_bytes()
    missing = [k for k in MSM_KERNELS if k not in scratch]
    assert not missing, missing
    bad = {k: scratch[k] for k in ZERO_SCRATCH if scratch[k] != 0}
    assert not bad, "scratch bytes per lane in the bucket accumulation / reduction kernels: %s" % bad
