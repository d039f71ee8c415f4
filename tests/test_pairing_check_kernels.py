"""CPU-only: the pairing-product kernels (per-pair validity fold, segmented Fp12 product) exist in the built library, and the
segmented product keeps its running value and operands without scratch (0 bytes per lane)."""
from tests.library_support import scratch_bytes

PCHECK_KERNELS = ("k_pair_ok", "k_fp12_seg_prod")


def test_pairing_check_kernels_built_and_seg_prod_without_scratch():
    scratch = scratch_bytes()
    missing = [k for k in PCHECK_KERNELS if k not in scratch]
    assert not missing, missing
    assert scratch["k_fp12_seg_prod"] == 0, "scratch bytes per lane in k_fp12_seg_prod: %d" % scratch["k_fp12_seg_prod"]
