"""CPU-only: the kernels of the checked signature aggregation over a registered key set exist in the built library, and the
byte-moving ones (the rows, the gather of the fallback's keys) keep everything in registers."""
from tests.library_support import scratch_bytes

KA_KERNELS = ("k_ka_scan", "k_ka_rows", "k_ka_gather_keys")


def test_keyset_aggregate_kernels_built_and_their_scratch():
    scratch = scratch_bytes()
    missing = [k for k in KA_KERNELS if k not in scratch]
    assert not missing, missing
    for k in ("k_ka_rows", "k_ka_gather_keys"):
        assert scratch[k] == 0, "scratch bytes per lane in %s: %d" % (k, scratch[k])
