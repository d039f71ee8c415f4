"""CPU-only: the kernels of the key-set FastAggregateVerify by random linear combination per message exist in the built library,
the G2 weight kernel -- the hot one -- keeps its accumulator, the point and the sum in registers (the scratch the build reports
for it, DESIGN.md 6m: 0 bytes per lane), as do the G1 weight kernel and the gather, and the library exports what
include/blsbn254.h declares for the feature (tests/test_abi.py holds that for every symbol; restated for the new ones)."""
import ctypes
import os
import re

from tests.library_support import declared_symbols, scratch_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KSR_KERNELS = ("k_ksr_elig", "k_ksr_weigh_g1", "k_ksr_weigh_g2", "k_ksr_chunks", "k_ksr_gather")
KSR_SYMBOLS = ("blsbn254_keyset_fast_aggregate_verify_batch_rlc", "blsbn254_keyset_committee_fast_aggregate_verify_batch_rlc",
               "blsbn254_set_keyset_rlc_group", "blsbn254_keyset_rlc_stats")
G2_WEIGHT_SCRATCH = 0                                                   # bytes per lane, as the build reports and DESIGN.md 6m states


def test_keyset_rlc_kernels_built_and_their_scratch():
    scratch = scratch_bytes()
    missing = [k for k in KSR_KERNELS + ("k_g1_seg_sum", "k_g2_seg_sum", "k_g2p_to_bytes") if k not in scratch]
    assert not missing, missing
    assert scratch["k_ksr_weigh_g2"] == G2_WEIGHT_SCRATCH, "scratch bytes per lane in k_ksr_weigh_g2: %d" % scratch["k_ksr_weigh_g2"]
    for k in ("k_ksr_weigh_g1", "k_ksr_gather"):
        assert scratch[k] == 0, "scratch bytes per lane in %s: %d" % (k, scratch[k])


def test_design_states_the_scratch_of_the_g2_weight_kernel():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"k_ksr_weigh_g2[^\n]*?(\d+) bytes of scratch", text)
    assert m and int(m.group(1)) == G2_WEIGHT_SCRATCH


def test_keyset_rlc_entry_points_declared_and_exported():
    import blsbn254_loader
    M = blsbn254_loader.load()
    declared = declared_symbols()
    lib = ctypes.CDLL(M.library_path())
    for s in KSR_SYMBOLS:
        assert s in declared and hasattr(lib, s), s
    for name in ("keyset_fast_aggregate_verify_batch_rlc", "keyset_committee_fast_aggregate_verify_batch_rlc", "set_keyset_rlc_group", "keyset_rlc_stats"):
        assert callable(getattr(M.Engine, name))
