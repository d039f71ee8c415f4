"""CPU-only: the kernels of the pairing-product checks over ragged groups by random linear combination exist in the built library,
the weight kernel -- the hot one, two interleaved double-and-add chains per lane -- needs no more scratch than k_rlc2_prep, the
kernel its compile policy is taken from, in the same build, and the library exports what include/blsbn254.h declares for the
feature (tests/test_abi.py holds that for every symbol; restated for the new ones)."""
import ctypes

from tests.library_support import declared_symbols, kernel_table, library_path_built, scratch_bytes
from tests.pairing_check_rlc_support import PCR_KERNELS, PCR_STATS, PCR_SYMBOLS


def test_pairing_check_rlc_kernels_built():
    table = {r["name"] for r in kernel_table(library_path_built())}
    missing = [k for k in PCR_KERNELS + ("k_agr_bits", "k_g1_seg_sum", "k_g1p_to_h_affine", "k_fp12_seg_prod", "k_g2_prepare") if k not in table]
    assert not missing, missing


def test_weight_kernel_scratch_at_most_that_of_rlc2_prep():
    scratch = scratch_bytes()
    print("scratch bytes per lane: k_pcr_weigh %d, k_rlc2_prep %d, k_pcr_pairs %d, k_pcr_eq %d" %
          (scratch["k_pcr_weigh"], scratch["k_rlc2_prep"], scratch["k_pcr_pairs"], scratch["k_pcr_eq"]))
    assert scratch["k_pcr_weigh"] <= scratch["k_rlc2_prep"]


def test_pairing_check_rlc_entry_points_declared_and_exported():
    import blsbn254_loader
    M = blsbn254_loader.load()
    declared = declared_symbols()
    lib = ctypes.CDLL(library_path_built())
    for s in PCR_SYMBOLS:
        assert s in declared and hasattr(lib, s), s
        assert s in M.engine.PROTOTYPES, s
    for name in ("pairing_check_batch_rlc", "set_pairing_check_rlc_segments", "pairing_check_rlc_stats"):
        assert callable(getattr(M.Engine, name))
    assert len(PCR_STATS) == 8
