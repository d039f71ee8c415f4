"""The built library contains the four hashing kernels that take the expander as an argument (k_hash_keccak.hip), Keccak-f[1600]
is a function of its own in their code object, and the default path is untouched: the rows of the four XMD-SHA-256 kernels are
the parent commit's.  Read from the gfx950 code objects through scripts/kernel_resources.py.  No GPU needed."""
from tests.library_support import demangled, instruction_counts, kernel_table, library_path_built

# What the build of 2026-10-20 (hipcc -O3, Makefile HASHX_FLAGS) shows for the new kernels: VGPRs, scratch bytes per lane,
# instructions of the kernel's own symbol.  The first two are limits; the third is the base of the inlining bound below.
BUILT = {"k_hash_to_g1_x": (254, 592, 81447), "k_hash_to_g2_x": (491, 1328, 148964), "k_sign_x": (414, 624, 43998), "k_hash_to_scalar_x": (152, 224, 7498)}
# keccak_f as built: 361 instructions (the 24 rounds are a loop over one body).  Every keccak_byte / keccak_finish / keccak_squeeze
# has a call site of it: 20 per XMD expansion, 7 per XOF expansion, so a kernel that inlined it would grow by at least
# 27 x 361 = 9.7 k instructions per copy of expand_message it holds (three in k_hash_to_g1_x: +36 %; one in k_hash_to_scalar_x:
# +130 %).  A rebuild of one source with one compiler gives the same counts (the parent rows below are compared for equality); the
# 10 % headroom is room for another compiler release and still far below what inlining would add.
HEADROOM = 1.10
# The rows of the default path in the parent commit (d22f326), built here the same day with the same compiler: registers, AGPRs,
# spills, scratch, LDS, and the instruction count of the kernel's symbol.  Any difference means the default path was touched.
PARENT = {"k_hash_to_g1": {"vgpr": 254, "agpr": 0, "vgpr_spills": 0, "sgpr_spills": 0, "scratch": 592, "lds": 0, "instructions": 60553},
          "k_hash_to_g2": {"vgpr": 512, "agpr": 256, "vgpr_spills": 7, "sgpr_spills": 2, "scratch": 4000, "lds": 0, "instructions": 10080},
          "k_sign": {"vgpr": 292, "agpr": 36, "vgpr_spills": 0, "sgpr_spills": 0, "scratch": 1328, "lds": 0, "instructions": 19562},
          "k_hash_to_scalar": {"vgpr": 93, "agpr": 0, "vgpr_spills": 0, "sgpr_spills": 0, "scratch": 128, "lds": 0, "instructions": 1850}}


def rows():
    path = library_path_built()
    sizes = instruction_counts(path)
    return {r["name"]: dict(r, instructions=sizes[r["symbol"]]) for r in kernel_table(path)}, sizes


def test_the_expander_kernels_exist_within_the_built_figures():
    table, _ = rows()
    for name, (vgpr, scratch, _) in BUILT.items():
        assert name in table, (name, sorted(table))
        r = table[name]
        assert r["vgpr"] <= vgpr and r["scratch"] <= scratch and r["vgpr_spills"] == 0, (name, r)
        assert r["instructions"] >= 200, "suspiciously small kernel (undefined behaviour in the source?): %s" % name


def test_keccak_f_is_a_function_not_inlined_per_call_site():
    table, sizes = rows()
    names = demangled(sizes)
    f = [n for s, n in sizes.items() if names[s] == "bn::keccak_f"]
    assert len(f) == 1 and 200 <= f[0] <= 1000, f            # one body, about one round long
    for name, (_, _, built) in BUILT.items():
        assert table[name]["instructions"] <= built * HEADROOM, (name, table[name]["instructions"], built)


def test_the_default_kernels_are_the_parents():
    table, _ = rows()
    for name, want in PARENT.items():
        assert {k: table[name][k] for k in want} == want, name


def test_the_library_exports_the_setter_and_the_package_the_ids():
    import blsbn254_loader
    M = blsbn254_loader.load()
    lib = M.load_library()
    assert hasattr(lib, "blsbn254_set_expander") and hasattr(lib, "blsbn254_get_expander")
    assert (M.EXPAND_XMD_SHA256, M.EXPAND_XMD_KECCAK256, M.EXPAND_XMD_SHA3_256, M.EXPAND_XOF_SHAKE128, M.EXPAND_XOF_SHAKE256) == (0, 1, 2, 3, 4)
    assert lib.blsbn254_set_expander(None, 1) == -1 and lib.blsbn254_get_expander(None) == -1
