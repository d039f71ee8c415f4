"""The built library contains the inflate kernels, and they are real code: the instruction count that
tests/test_kernel_sanity.py::test_no_degenerate_kernels applies to every kernel, read from the gfx950 code objects through
scripts/kernel_resources.py.  No GPU needed."""
from tests.library_support import instruction_counts, kernel_table, library_path_built


def library():
    import blsbn254_loader
    return blsbn254_loader.load(), library_path_built()


def test_inflate_kernels_are_in_the_library_and_not_degenerate():
    _, path = library()
    sizes = instruction_counts(path)                                      # by symbol: the mangled names
    scratch = {r["symbol"]: r["scratch"] for r in kernel_table(path)}
    for k in ("k_g1_inflate", "k_g2_inflate"):
        names = [s for s in sizes if k in s]
        assert len(names) == 1, (k, sorted(sizes))
        assert sizes[names[0]] >= 200, "suspiciously small kernel (undefined behaviour in the source?): %s %d" % (names[0], sizes[names[0]])
        # the table of fp_pow_pm3_4 (14 field elements of 36 bytes) lives in scratch, and nothing else should
        assert 504 <= scratch[[s for s in scratch if k in s][0]] <= 1024, scratch


def test_the_library_exports_the_compressed_entry_points():
    M, _ = library()
    lib = M.load_library()
    for name in ("blsbn254_g1_inflate_batch", "blsbn254_g2_inflate_batch", "blsbn254_verify_batch_compressed", "blsbn254_verify_batch_rlc_compressed",
                 "blsbn254_keyset_create_compressed", "blsbn254_keyset_fast_aggregate_verify_batch_compressed"):
        assert hasattr(lib, name), name
