"""The built library contains the kernels of the wire-format aggregation and merge calls, and they are real code: the instruction
count that tests/test_kernel_sanity.py::test_no_degenerate_kernels applies to every kernel, and the scratch of the two scans
(the table of the square-root chain and nothing else), read from the gfx950 code objects through scripts/kernel_resources.py.
No GPU needed."""
import re

from tests.library_support import instruction_counts, kernel_table, library_path_built
KERNELS = ("k_ka_scan_wire", "k_kca_scan_wire", "k_g1p_to_wire")


def library():
    import blsbn254_loader
    return blsbn254_loader.load(), library_path_built()


def test_wire_kernels_are_in_the_library_and_not_degenerate():
    _, path = library()
    sizes = instruction_counts(path)                                      # by symbol: the mangled names
    scratch = {r["symbol"]: r["scratch"] for r in kernel_table(path)}
    spills = {r["symbol"]: r["vgpr_spills"] + r["sgpr_spills"] for r in kernel_table(path)}
    for k in KERNELS:
        names = [s for s in sizes if re.search(r"\d%s(?![a-z_0-9])" % k, s)]          # the mangled name: <length><name><parameters>
        assert len(names) == 1, (k, sorted(sizes))
        assert sizes[names[0]] >= 200, "suspiciously small kernel (undefined behaviour in the source?): %s %d" % (names[0], sizes[names[0]])
        assert spills[names[0]] == 0, (k, spills)
        if k != "k_g1p_to_wire":
            # the table of fp_pow_pm3_4 (14 field elements of 36 bytes) lives in scratch, and nothing else should
            assert 504 <= scratch[names[0]] <= 1024, (k, scratch)


def test_the_library_exports_the_wire_format_entry_points():
    M, _ = library()
    lib = M.load_library()
    for name in ("blsbn254_keyset_aggregate_checked_batch_compressed", "blsbn254_keyset_committee_aggregate_checked_batch_compressed",
                 "blsbn254_keyset_merge_checked_batch_compressed", "blsbn254_keyset_committee_merge_checked_batch_compressed",
                 "blsbn254_keyset_committee_fast_aggregate_verify_batch_compressed"):
        assert hasattr(lib, name), name
