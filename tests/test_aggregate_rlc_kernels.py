"""CPU-only: the kernels of the aggregate verify over ragged groups by random linear combination exist in the built library, the
weight kernel -- the hot one, two interleaved double-and-add chains per lane -- needs no more scratch than k_rlc2_prep, the kernel
it is modelled on, in the same build, and the library exports what include/blsbn254.h declares for the feature
(tests/test_abi.py holds that for every symbol; restated for the new ones)."""
import ctypes

from tests.aggregate_rlc_support import AGR_KERNELS, AGR_STATS, AGR_SYMBOLS
from tests.library_support import declared_symbols, kernel_table, library_path_built, scratch_bytes


def test_aggregate_rlc_kernels_built():
    table = {r["name"] for r in kernel_table(library_path_built())}
    missing = [k for k in AGR_KERNELS + ("k_g1_seg_sum", "k_g1p_to_h_affine", "k_fp12_seg_prod", "k_fp12_mul_elem") if k not in table]
    assert not missing, missing


def test_weight_kernel_scratch_at_most_that_of_rlc2_prep():
    scratch = scratch_bytes()
    print("scratch bytes per lane: k_agr_weigh %d, k_rlc2_prep %d, k_agr_group %d" % (scratch["k_agr_weigh"], scratch["k_rlc2_prep"], scratch["k_agr_group"]))
    assert scratch["k_agr_weigh"] <= scratch["k_rlc2_prep"]


def test_aggregate_rlc_entry_points_declared_and_exported():
    import blsbn254_loader
    M = blsbn254_loader.load()
    declared = declared_symbols()
    lib = ctypes.CDLL(library_path_built())
    for s in AGR_SYMBOLS:
        assert s in declared and hasattr(lib, s), s
        assert s in M.engine.PROTOTYPES, s
    for name in ("aggregate_verify_batch_rlc", "aggregate_verify_batch_rlc_flat", "set_aggregate_rlc_segments", "aggregate_rlc_stats"):
        assert callable(getattr(M.Engine, name))
    assert len(AGR_STATS) == 8
