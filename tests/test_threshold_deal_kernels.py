"""CPU-only: the kernels of the threshold dealing side exist in the built library; the Horner evaluation in Fr keeps its
accumulator in registers (0 bytes of scratch per lane), and the evaluation in G2, which holds no window table, needs no more
scratch than k_g2_mul, the kernel it is measured against (both read from the same build)."""
from tests.library_support import scratch_bytes

TD_KERNELS = ("k_fr_coef_decode", "k_fr_poly_eval", "k_g2_poly_eval", "k_td_finish", "k_td_fr_encode", "k_td_g2_encode")


def test_threshold_deal_kernels_built_and_their_scratch():
    scratch = scratch_bytes()
    missing = [k for k in TD_KERNELS + ("k_g2_mul",) if k not in scratch]
    assert not missing, missing
    assert scratch["k_fr_poly_eval"] == 0, "scratch bytes per lane in k_fr_poly_eval: %d" % scratch["k_fr_poly_eval"]
    assert scratch["k_g2_poly_eval"] <= scratch["k_g2_mul"], "scratch bytes per lane: k_g2_poly_eval %d, k_g2_mul %d" % (
        scratch["k_g2_poly_eval"], scratch["k_g2_mul"])
