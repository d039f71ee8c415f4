"""CPU-only: the kernels of the threshold combine over many groups exist in the built library; the segmented Lagrange kernel
keeps its products and the three powers of its inversion in registers (0 bytes of scratch per lane), and the GLV scalar
multiplication, whose table lives in LDS, needs no more scratch than k_g1_mul, the kernel it competes with (both read from the
same build)."""
from tests.library_support import scratch_bytes

THB_KERNELS = ("k_lagrange_seg", "k_g1_smul_glv", "k_th_finish")


def test_threshold_batch_kernels_built_and_their_scratch():
    scratch = scratch_bytes()
    missing = [k for k in THB_KERNELS + ("k_g1_mul",) if k not in scratch]
    assert not missing, missing
    assert scratch["k_lagrange_seg"] == 0, "scratch bytes per lane in k_lagrange_seg: %d" % scratch["k_lagrange_seg"]
    assert scratch["k_g1_smul_glv"] <= scratch["k_g1_mul"], "scratch bytes per lane: k_g1_smul_glv %d, k_g1_mul %d" % (
        scratch["k_g1_smul_glv"], scratch["k_g1_mul"])
