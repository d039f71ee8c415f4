"""CPU-only: the kernels of the sums over a registered key set exist in the built library; k_ks_count (popcounts and masks
only) keeps everything in registers, and the two summing kernels need no more scratch per lane than the segmented G2 sum
they stand beside (k_g2_seg_sum) in the same build."""
from tests.library_support import scratch_bytes

KS_KERNELS = ("k_ks_count", "k_ks_word_sum", "k_ks_group_sum")


def test_keyset_kernels_built_and_their_scratch():
    scratch = scratch_bytes()
    missing = [k for k in KS_KERNELS + ("k_g2_seg_sum",) if k not in scratch]
    assert not missing, missing
    assert scratch["k_ks_count"] == 0, "scratch bytes per lane in k_ks_count: %d" % scratch["k_ks_count"]
    for k in ("k_ks_word_sum", "k_ks_group_sum"):
        assert scratch[k] <= scratch["k_g2_seg_sum"], "scratch bytes per lane: %s %d, k_g2_seg_sum %d" % (k, scratch[k], scratch["k_g2_seg_sum"])
