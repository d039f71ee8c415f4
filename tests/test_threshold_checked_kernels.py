"""CPU-only: the selection kernels of the checked threshold combine exist in the built library; the two that only move bytes
(k_tc_select: ranks and the compaction, k_tc_gather_c0: the groups' keys) keep everything in registers, 0 bytes of scratch
per lane."""
from tests.library_support import scratch_bytes

TC_KERNELS = ("k_tc_scan", "k_tc_select", "k_tc_gather_c0")


def test_threshold_checked_kernels_built_and_their_scratch():
    scratch = scratch_bytes()
    missing = [k for k in TC_KERNELS if k not in scratch]
    assert not missing, missing
    for k in ("k_tc_select", "k_tc_gather_c0"):
        assert scratch[k] == 0, "scratch bytes per lane in %s: %d" % (k, scratch[k])
