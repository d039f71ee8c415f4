"""CPU-only, on the built library: the aggregate verify over groups is declared, exported and wrapped; its kernels are in the
code object; the ragged two-pairs-per-lane Miller kernel (the loop body of k_miller_hpk2 behind a slot descriptor) needs no more
scratch than k_miller_hpk2 in the same build and no flat or serialised accesses beyond that kernel's; the signature placement
and the flag fold keep everything in registers."""
import ctypes
import os
import re

import pytest

from tests.library_support import M, library_path_built, lint_by_name, scratch_bytes  # noqa: F401 (M is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("blsbn254_aggregate_verify_batch", "blsbn254_aggregate_batch_stats")
KERNELS = ("k_agb_place_sigs", "k_miller_hpk2r", "k_agb_fold")


@pytest.fixture(scope="module")
def scratch():
    return scratch_bytes()


def test_header_declares_and_library_exports_both_symbols(M):
    text = open(os.path.join(ROOT, "include", "blsbn254.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, text), "not declared: " + s
    lib = ctypes.CDLL(library_path_built())
    for s in SYMBOLS:
        assert hasattr(lib, s), "missing export " + s


def test_engine_has_both_methods(M):
    assert callable(getattr(M.Engine, "aggregate_verify_batch", None))
    assert callable(getattr(M.Engine, "aggregate_batch_stats", None))


def test_kernels_are_in_the_code_object(scratch):
    missing = [k for k in KERNELS if k not in scratch]
    assert not missing, missing


def test_ragged_miller_kernel_needs_no_more_scratch_than_the_dense_one(scratch):
    print("scratch bytes per lane: k_miller_hpk2r %d, k_miller_hpk2 %d" % (scratch["k_miller_hpk2r"], scratch["k_miller_hpk2"]))
    assert scratch["k_miller_hpk2r"] <= scratch["k_miller_hpk2"]


def test_placement_and_fold_without_scratch(scratch):
    bad = {k: scratch[k] for k in ("k_agb_place_sigs", "k_agb_fold") if scratch[k] != 0}
    assert not bad, "scratch bytes per lane: %s" % bad


def test_ragged_miller_kernel_has_no_flat_or_serialised_accesses_beyond_the_dense_one(M):
    by_name = lint_by_name(M.library_path())
    r, d = by_name["k_miller_hpk2r"], by_name["k_miller_hpk2"]
    print("k_miller_hpk2r: %s; k_miller_hpk2: %s" % (dict(r), dict(d)))
    assert r["flat"] <= d["flat"]
    assert r["readfirstlane"] <= d["readfirstlane"]
    assert r["waterfall_loops"] <= d["waterfall_loops"]
