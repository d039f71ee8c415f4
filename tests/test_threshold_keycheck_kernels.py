"""CPU-only: the kernels of the key-share check exist in the built library, and the check kernel, which holds less state (an
accumulator, one table entry, the key share) than the evaluation it follows, needs no more scratch than k_g2_poly_eval (both read
from the same build).  The check kernel reads the table through one base and a per-lane offset: no read-first-lane loop, no flat
access.  The scratch of k_g2gen_table, which runs once per context, is reported in DESIGN.md 6r and not limited here."""
from tests.library_support import library_path_built, lint_by_name, scratch_bytes

KC_KERNELS = ("k_g2gen_table", "k_td_key_check", "k_td_key_bits")


def test_threshold_keycheck_kernels_built_and_their_scratch():
    scratch = scratch_bytes()
    missing = [k for k in KC_KERNELS + ("k_g2_poly_eval",) if k not in scratch]
    assert not missing, missing
    assert scratch["k_td_key_check"] <= scratch["k_g2_poly_eval"], "scratch bytes per lane: k_td_key_check %d, k_g2_poly_eval %d" % (
        scratch["k_td_key_check"], scratch["k_g2_poly_eval"])


def test_check_kernel_addresses_the_table_by_base_and_lane_offset():
    c = lint_by_name(library_path_built())["k_td_key_check"]
    assert c["readfirstlane"] == 0 and c["waterfall_loops"] == 0 and c["flat"] == 0, dict(c)
