"""CPU-only: the kernels of the checked signature aggregation per committee of a registered key set exist in the built library;
the rows, the resolve and the key gather (searches, bit tests and copies only) keep everything in registers, and the scan, whose
candidate test evaluates the curve equation, needs no more scratch per lane than the scan of the full-width call (k_ka_scan) in
the same build.  The library still exports exactly what include/blsbn254.h declares (tests/test_abi.py holds that; restated for
the new symbols)."""
import ctypes

from tests.library_support import declared_symbols, scratch_bytes

KCA_KERNELS = ("k_kca_scan", "k_kca_rows", "k_kca_resolve")
KCA_SYMBOLS = ("blsbn254_keyset_committee_aggregate_checked_batch", "blsbn254_keyset_committee_aggregate_stats")


def test_keyset_committee_aggregate_kernels_built_and_their_scratch():
    scratch = scratch_bytes()
    missing = [k for k in KCA_KERNELS + ("k_ka_scan", "k_ka_gather_keys") if k not in scratch]
    assert not missing, missing
    for k in ("k_kca_rows", "k_kca_resolve", "k_ka_gather_keys"):
        assert scratch[k] == 0, "scratch bytes per lane in %s: %d" % (k, scratch[k])
    assert scratch["k_kca_scan"] <= scratch["k_ka_scan"], "scratch bytes per lane: k_kca_scan %d, k_ka_scan %d" % (scratch["k_kca_scan"], scratch["k_ka_scan"])


def test_committee_aggregate_entry_points_declared_and_exported():
    import blsbn254_loader
    M = blsbn254_loader.load()
    declared = declared_symbols()
    lib = ctypes.CDLL(M.library_path())
    for s in KCA_SYMBOLS:
        assert s in declared and hasattr(lib, s), s
