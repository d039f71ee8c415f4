"""CPU-only: the kernels of the checked merge of partial aggregates over a registered key set exist in the built library, and
the ones that only move bits (the selection, a wave per group with its union in a register or in the merged row, and the pass
over the points) keep everything in registers."""
from tests.library_support import scratch_bytes

KM_KERNELS = ("k_km_sig", "k_km_select", "k_km_points")


def test_keyset_merge_kernels_built_and_their_scratch():
    scratch = scratch_bytes()
    missing = [k for k in KM_KERNELS if k not in scratch]
    assert not missing, missing
    for k in ("k_km_select", "k_km_points"):
        assert scratch[k] == 0, "scratch bytes per lane in %s: %d" % (k, scratch[k])
