"""CPU-only: the selection kernel of the checked merge of partial aggregates per committee of a registered key set exists in the
built library and keeps everything in registers (votes, bit tests and byte stores only), as the full-width selection beside it
does.  The library still exports exactly what include/blsbn254.h declares (tests/test_abi.py holds that; restated for the new
symbols)."""
import ctypes

from tests.library_support import declared_symbols, scratch_bytes

KCM_SYMBOLS = ("blsbn254_keyset_committee_merge_checked_batch", "blsbn254_keyset_committee_merge_stats")


def test_keyset_committee_merge_kernel_built_and_its_scratch():
    scratch = scratch_bytes()
    missing = [k for k in ("k_kcm_select", "k_km_select", "k_km_sig", "k_km_points") if k not in scratch]
    assert not missing, missing
    assert scratch["k_kcm_select"] == 0, "scratch bytes per lane in k_kcm_select: %d" % scratch["k_kcm_select"]


def test_committee_merge_entry_points_declared_and_exported():
    import blsbn254_loader
    M = blsbn254_loader.load()
    declared = declared_symbols()
    lib = ctypes.CDLL(M.library_path())
    for s in KCM_SYMBOLS:
        assert s in declared and hasattr(lib, s), s
