"""CPU-only: the two kernels of the distinct-message rule (k_msg_distinct.hip) exist in the built library -- the insert kernel, one
probe loop over integers, with no scratch, no spills and no LDS; the key kernel without spills (its scratch, the stack of the
inversion it shares with the hash kernels, is recorded in DESIGN.md 6v, not bounded here) -- the library exports what
include/blsbn254.h declares for the feature, and the kernels of the two aggregate pipelines the stage is attached to are the
parent commit's.  Read from the gfx950 code objects through scripts/kernel_resources.py.  No GPU needed."""
import ctypes

from tests.library_support import declared_symbols, instruction_counts, kernel_table, library_path_built
from tests.msg_distinct_support import MD_KERNELS, MD_STATS, MD_SYMBOLS

# The rows of the aggregate kernels in the parent commit (589b1c6), built with the same compiler: registers, AGPRs, spills,
# scratch, LDS, and the instruction count of the kernel's symbol.  Any difference means an existing kernel was touched.
# A compiler update changes these rows too: then print them from a build of the parent commit with that compiler --
#   for r in kernel_table(library_path_built()): print(r["name"], r, instruction_counts(library_path_built())[r["symbol"]])
# (tests/library_support.py) -- and replace the rows below with what it shows; the same rows from a build of THIS tree must match.
PARENT = {"k_agb_place_sigs": {"vgpr": 65, "agpr": 0, "vgpr_spills": 0, "sgpr_spills": 0, "scratch": 0, "lds": 0, "instructions": 2661},
          "k_miller_hpk2r": {"vgpr": 508, "agpr": 252, "vgpr_spills": 30, "sgpr_spills": 15, "scratch": 0, "lds": 147456, "instructions": 177862},
          "k_agb_fold": {"vgpr": 8, "agpr": 0, "vgpr_spills": 0, "sgpr_spills": 0, "scratch": 0, "lds": 0, "instructions": 370},
          "k_agr_group": {"vgpr": 256, "agpr": 0, "vgpr_spills": 43, "sgpr_spills": 0, "scratch": 288, "lds": 0, "instructions": 9303},
          "k_agr_weigh": {"vgpr": 256, "agpr": 0, "vgpr_spills": 23, "sgpr_spills": 0, "scratch": 96, "lds": 0, "instructions": 13860},
          "k_agr_items": {"vgpr": 11, "agpr": 0, "vgpr_spills": 0, "sgpr_spills": 0, "scratch": 0, "lds": 0, "instructions": 230},
          "k_agr_bits": {"vgpr": 4, "agpr": 0, "vgpr_spills": 0, "sgpr_spills": 0, "scratch": 0, "lds": 0, "instructions": 306}}


def rows():
    path = library_path_built()
    sizes = instruction_counts(path)
    return {r["name"]: dict(r, instructions=sizes[r["symbol"]]) for r in kernel_table(path)}


def test_the_new_kernels_exist():
    table = rows()
    for name in MD_KERNELS:
        assert name in table, (name, sorted(table))
        r = table[name]
        print(name, {k: r[k] for k in ("vgpr", "agpr", "vgpr_spills", "sgpr_spills", "scratch", "lds", "instructions")})
        assert r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["lds"] == 0, (name, r)
        assert r["instructions"] >= 100, "suspiciously small kernel (undefined behaviour in the source?): %s" % name
    assert table["k_md_insert"]["scratch"] == 0, table["k_md_insert"]
    assert table["k_md_insert"]["vgpr"] <= 128, table["k_md_insert"]      # four waves per SIMD at the least: the kernel waits on memory


def test_the_aggregate_kernels_are_the_parents():
    table = rows()
    for name, want in PARENT.items():
        assert {k: table[name][k] for k in want} == want, name


def test_entry_points_declared_and_exported():
    import blsbn254_loader
    M = blsbn254_loader.load()
    declared = declared_symbols()
    lib = ctypes.CDLL(library_path_built())
    for s in MD_SYMBOLS:
        assert s in declared and hasattr(lib, s), s
        assert s in M.engine.PROTOTYPES, s
    for name in ("hash_distinct_batch", "aggregate_verify_batch_distinct", "aggregate_verify_batch_distinct_flat", "aggregate_verify_batch_rlc_distinct",
                 "aggregate_verify_batch_rlc_distinct_flat", "msg_distinct_stats"):
        assert callable(getattr(M.Engine, name))
    assert len(MD_STATS) == 4
