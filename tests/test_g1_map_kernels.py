"""The built library contains the two kernels of the try-and-increment map (k_hash_tai.hip), exports the setter, and the
SVDW path is untouched: the rows of k_hash_to_g1, k_hash_to_g1_x, k_sign and k_sign_x are the parent commit's.  Read from the
gfx950 code objects through scripts/kernel_resources.py.  No GPU needed.  The new kernels' scratch bytes are recorded in DESIGN.md
6u, not bounded here."""
from tests.library_support import instruction_counts, kernel_table, library_path_built

NEW = ("k_hash_to_g1_tai", "k_sign_tai")
# The rows of the SVDW kernels in the parent commit (7ea6412), built with the same compiler: registers, AGPRs, spills, scratch,
# LDS, and the instruction count of the kernel's symbol.  Any difference means the default path was touched.
PARENT = {"k_hash_to_g1": {"vgpr": 254, "agpr": 0, "vgpr_spills": 0, "sgpr_spills": 0, "scratch": 592, "lds": 0, "instructions": 60553},
          "k_hash_to_g1_x": {"vgpr": 254, "agpr": 0, "vgpr_spills": 0, "sgpr_spills": 0, "scratch": 592, "lds": 0, "instructions": 81447},
          "k_sign": {"vgpr": 292, "agpr": 36, "vgpr_spills": 0, "sgpr_spills": 0, "scratch": 1328, "lds": 0, "instructions": 19562},
          "k_sign_x": {"vgpr": 414, "agpr": 158, "vgpr_spills": 0, "sgpr_spills": 0, "scratch": 624, "lds": 0, "instructions": 43998}}


def rows():
    path = library_path_built()
    sizes = instruction_counts(path)
    return {r["name"]: dict(r, instructions=sizes[r["symbol"]]) for r in kernel_table(path)}


def test_the_new_kernels_exist():
    table = rows()
    for name in NEW:
        assert name in table, (name, sorted(table))
        r = table[name]
        assert r["vgpr_spills"] == 0 and r["lds"] == 0, (name, r)
        assert r["instructions"] >= 200, "suspiciously small kernel (undefined behaviour in the source?): %s" % name


def test_the_svdw_kernels_are_the_parents():
    table = rows()
    for name, want in PARENT.items():
        assert {k: table[name][k] for k in want} == want, name


def test_the_library_exports_the_setter_and_the_package_the_ids():
    import blsbn254_loader
    M = blsbn254_loader.load()
    lib = M.load_library()
    assert hasattr(lib, "blsbn254_set_g1_map") and hasattr(lib, "blsbn254_get_g1_map")
    assert (M.G1MAP_SVDW, M.G1MAP_TAI_DIGEST, M.G1MAP_TAI_HASH) == (0, 1, 2)
    assert lib.blsbn254_set_g1_map(None, 1) == -1 and lib.blsbn254_get_g1_map(None) == -1
