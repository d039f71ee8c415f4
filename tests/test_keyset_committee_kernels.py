"""CPU-only: the kernels of the committees over a registered key set exist in the built library; the count, the committee words
and the weights (popcounts, masks and integer sums only) keep everything in registers, and the two kernels that do curve
arithmetic need no more scratch per lane than the segmented G2 sum that reduces their partials (k_g2_seg_sum) in the same
build.  The library still exports exactly what include/blsbn254.h declares (tests/test_abi.py holds that; restated for the new
symbols)."""
import ctypes

from tests.library_support import declared_symbols, scratch_bytes

KC_KERNELS = ("k_kc_words", "k_kc_count", "k_kc_word_sum", "k_kc_finish", "k_kc_weight")
KC_SYMBOLS = ("blsbn254_keyset_set_committees", "blsbn254_keyset_committee_count", "blsbn254_keyset_committee_sum_batch",
              "blsbn254_keyset_committee_fast_aggregate_verify_batch", "blsbn254_keyset_committee_weight_batch", "blsbn254_keyset_committee_stats")


def test_keyset_committee_kernels_built_and_their_scratch():
    scratch = scratch_bytes()
    missing = [k for k in KC_KERNELS + ("k_g2_seg_sum",) if k not in scratch]
    assert not missing, missing
    for k in ("k_kc_count", "k_kc_words", "k_kc_weight"):
        assert scratch[k] == 0, "scratch bytes per lane in %s: %d" % (k, scratch[k])
    for k in ("k_kc_word_sum", "k_kc_finish"):
        assert scratch[k] <= scratch["k_g2_seg_sum"], "scratch bytes per lane: %s %d, k_g2_seg_sum %d" % (k, scratch[k], scratch["k_g2_seg_sum"])


def test_committee_entry_points_declared_and_exported():
    import blsbn254_loader
    M = blsbn254_loader.load()
    declared = declared_symbols()
    lib = ctypes.CDLL(M.library_path())
    for s in KC_SYMBOLS:
        assert s in declared and hasattr(lib, s), s
