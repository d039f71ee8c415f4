"""GPU tests (MI355X) of every device form of the Miller loop and of the key preparation on EDGE-CASE AND OFF-CURVE points
(tests/point_cases.py: limb-boundary coordinates, both signs, points of the twist outside the r-torsion, coordinates on no curve,
identities by encoding, tiled without a period), byte for byte against the oracle, whose raw calls have the same domain: they
decode their operands and check nothing else.  Every assertion about a form also asserts, from the engine's launch record, that
this Miller kernel ran once and no other Miller kernel ran.  The sizes at which a form takes over are those of miller_to_ws
(host.hip), launch_g2_prepare, launch_miller_prepared and verify_chunk_dev (host_verify.hip) and, for
blsbn254_multi_miller_loop_prepared, launch_miller_raw (host_aggregate.hip; the other callers: tests/test_gpu_aggregate_forms.py)."""
import numpy as np
import pytest

from tests import point_cases as C
from tests import synth
from tests.gpu_support import ENGINES, MILLER_KERNELS, PREP_KERNELS, eng, engines, launches, M  # noqa: F401 (fixtures)
from tests.helpers import b32, bits_of

pytestmark = pytest.mark.gpu
WIDE_MAX = 2048                                   # wide_fe_max of host_common.h: the prepared-key forms; variable points take half


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def table(oracle, pyref):
    return C.pairs(oracle, pyref)


def miller_form(name, n, cus):
    """the kernel miller_to_ws launches for n variable-point pairs on that engine"""
    if name == "default" and n <= WIDE_MAX // 2:
        return "miller_wide_1"
    return "miller_tri_1" if name != "lane" and n <= cus * 64 else "miller_1"


def prepared_form(n):
    """the kernel of blsbn254_multi_miller_loop_prepared on an engine with the wave-per-pair kernels on"""
    return "miller_wide_1p" if n <= WIDE_MAX else "miller_hpk2p"


def verify_form(name, n, cus, auto_prepare=True):
    """the Miller kernel of verify_batch for n tuples with few distinct keys (verify_chunk_dev, launch_miller_prepared)"""
    wide = name == "default" and n <= WIDE_MAX
    tri = name != "lane" and n <= cus * 64
    if not auto_prepare or not (n >= 1024 or wide or tri):
        return "miller_verify"                    # the exact per-tuple path: what small batches take without wide or quad kernels
    return "miller_wide_prepared" if wide else "miller_tri_prepared" if tri else "miller_prepared"


def size_of(size, cus):
    return size if isinstance(size, int) else cus * 64 + (size == "tri_max + 1")


def assert_rows(got, want, width, v, names, what):
    """got == want, or how many rows of `width` bytes differ and, for the first few, the position, the index and the case names"""
    if got != want:
        assert len(got) == len(want), what
        bad = [i for i in range(len(want) // width) if got[width * i:width * i + width] != want[width * i:width * i + width]]
        raise AssertionError("%s: %d of %d values differ from the oracle, the first at %s" % (what, len(bad), len(want) // width,
                                                                                         [(i, int(v[i]), names[v[i]]) for i in bad[:8]]))


def check_tiled_pairs(e, table, n, want_kernel):
    names, g1s, g2s, mls, gts = table
    assert all(count < 0.02 * n for count in C.repeats(n).values())       # the input condition, for the sizes this device gives
    g1, g2, v = C.tile(g1s, n), C.tile(g2s, n), C.spread(n)
    got, ran = launches(e, lambda: e.miller_loop_batch(g1, g2, n), MILLER_KERNELS)
    assert ran == {want_kernel: 1}
    assert_rows(got, C.tile(mls, n), 384, v, names, "miller_loop_batch, n = %d" % n)
    got, ran = launches(e, lambda: e.pairing_batch(g1, g2, n), MILLER_KERNELS)
    assert ran == {want_kernel: 1}
    assert_rows(got, C.tile(gts, n), 384, v, names, "pairing_batch, n = %d" % n)


# ---------------- variable points
@pytest.mark.parametrize("name,size", [(name, n) for name in ENGINES for n in (1, 63, 64, 65, 251)] +
                         [("default", s) for s in (1024, 1025, "tri_max", "tri_max + 1")])
def test_variable_point_forms_on_edge_case_points(engines, table, oracle, pyref, cus, name, size):
    """one pair, a partial and a full 64-pair workgroup of the quad grid, a second workgroup, every pair of the tile, and each
    production switch-over from both sides (1024 | 1025: wave per pair | quad; tri_max | tri_max + 1: quad | one lane per pair)"""
    n = size_of(size, cus)
    e = engines[name]
    check_tiled_pairs(e, table, n, miller_form(name, n, cus))
    if n == 1:                                        # the tile's first pair is a named one: a plain random pair alone too
        names, g1s, g2s, mls, gts = table
        k = C.n_named(oracle, pyref)
        got, ran = launches(e, lambda: e.miller_loop_batch(g1s[k], g2s[k], 1), MILLER_KERNELS)
        assert ran == {miller_form(name, 1, cus): 1} and got == mls[k]
        got, ran = launches(e, lambda: e.pairing_batch(g1s[k], g2s[k], 1), MILLER_KERNELS)
        assert ran == {miller_form(name, 1, cus): 1} and got == gts[k]


# ---------------- products
@pytest.fixture(scope="module")
def products(oracle, table):
    """n -> oracle.multi_miller_loop over the tile of n pairs, computed on first use and kept for the module"""
    names, g1s, g2s, mls, gts = table
    made = {}

    def get(n):
        if n not in made:
            made[n] = oracle.multi_miller_loop(C.tile(g1s, n), C.tile(g2s, n), n)
        return made[n]
    return get


@pytest.mark.parametrize("name,n", [(name, n) for name in ENGINES for n in (1, 2, 65, 1025)])
def test_multi_miller_loop_over_the_tile(engines, table, products, cus, name, n):
    names, g1s, g2s, mls, gts = table
    e = engines[name]
    got, ran = launches(e, lambda: e.multi_miller_loop(C.tile(g1s, n), C.tile(g2s, n), n), MILLER_KERNELS)
    assert ran == {miller_form(name, n, cus): 1}
    assert got == products(n)


GROUP_SIZES = (0, 1, 2, 5, 0, 64, 65)
FIRST_OFFSET = 3


@pytest.mark.parametrize("name", ENGINES)
def test_multi_miller_loop_batch_over_ragged_groups(engines, table, oracle, cus, name):
    """groups of 0, 1, 2, 5, 0, 64 and 65 pairs of the tile behind three pairs that belong to no group: each group's product is the
    oracle's, an empty group gives one"""
    names, g1s, g2s, mls, gts = table
    e = engines[name]
    off = FIRST_OFFSET + np.concatenate([[0], np.cumsum(GROUP_SIZES)]).astype(np.uint64)
    total = int(off[-1])
    g1, g2, v = C.tile(g1s, total), C.tile(g2s, total), C.spread(total)
    got, ran = launches(e, lambda: e.multi_miller_loop_batch(g1, g2, off), MILLER_KERNELS)
    assert ran == {miller_form(name, total - FIRST_OFFSET, cus): 1}
    for g, size in enumerate(GROUP_SIZES):
        lo, hi = int(off[g]), int(off[g + 1])
        want = oracle.multi_miller_loop(g1[64 * lo:64 * hi], g2[128 * lo:128 * hi], size) if size else C.ONE_GT
        assert got[384 * g:384 * g + 384] == want, (g, size, [names[i] for i in v[lo:hi][:8]])


@pytest.mark.parametrize("name", ENGINES)
def test_pairing_check_on_cancelling_groups(engines, oracle, pyref, cus, name):
    """{(P, Q), (-P, Q)}: the bit is set for P an edge case of G1 and Q in the subgroup; cleared for Q on the twist outside the
    r-torsion, where the product of pairings IS one (by the oracle) and the torsion test alone clears it; cleared for a member
    off its curve"""
    e = engines[name]
    groups = C.check_groups(oracle, pyref)
    g1, g2 = b"".join(g for _, g, _, _ in groups), b"".join(g for _, _, g, _ in groups)
    off = np.arange(0, 2 * len(groups) + 1, 2, dtype=np.uint64)
    got, ran = launches(e, lambda: e.pairing_check_batch(g1, g2, off), MILLER_KERNELS)
    assert ran == {miller_form(name, 2 * len(groups), cus): 1}
    got = bits_of(got, len(groups))
    kinds = set()
    for (label, p, q, want), bit in zip(groups, got):
        assert bit == want, label
        if "outside" in label:
            assert oracle.final_exponentiation(oracle.multi_miller_loop(p, q, 2), 1) == C.ONE_GT and not bit, label
        kinds.add((want, "outside" in label, "off_" in label))
    assert kinds == {(True, False, False), (False, True, False), (False, False, True)}
    # ... and the products themselves, through the call that does not check
    prods, ran = launches(e, lambda: e.multi_miller_loop_batch(g1, g2, off), MILLER_KERNELS)
    assert ran == {miller_form(name, 2 * len(groups), cus): 1}
    for g, (label, p, q, want) in enumerate(groups):
        assert prods[384 * g:384 * g + 384] == oracle.multi_miller_loop(p, q, 2), label


# ---------------- an operand that does not decode
@pytest.mark.parametrize("name", ENGINES)
def test_undecodable_operand_mid_batch(engines, table, pyref, M, cus, name):
    names, g1s, g2s, mls, gts = table
    e = engines[name]
    n, at = 300, 200
    g1, g2, v = C.tile(g1s, n), C.tile(g2s, n), C.spread(n)
    bad1 = bytearray(g1); bad1[64 * at:64 * at + 32] = b32(pyref.P)                # x = p
    bad2 = bytearray(g2); bad2[128 * at:128 * at + 32] = b32(pyref.P)              # x.c1 = p
    for bad, exc, args in ((bad1, M.InvalidG1Bytes, lambda b: (bytes(b), g2)), (bad2, M.InvalidG2Bytes, lambda b: (g1, bytes(b)))):
        with pytest.raises(exc):
            e.pairing_batch(*args(bad), n)
        with pytest.raises(exc):
            e.miller_loop_batch(*args(bad), n)
        with pytest.raises(exc):
            e.multi_miller_loop(*args(bad), n)
        got, ran = launches(e, lambda: e.pairing_batch(g1, g2, n), MILLER_KERNELS)       # the context is usable afterwards
        assert ran == {miller_form(name, n, cus): 1}
        assert_rows(got, C.tile(gts, n), 384, v, names, "pairing_batch after %s" % exc.__name__)


# ---------------- prepared keys
@pytest.fixture(scope="module")
def prepared_terms(oracle, pyref):
    """(g1 of n, idx of n, want) by n: the G1 cases cycled -- identities and off-curve ones included: they decode -- each against a
    valid key that moves on by one every time the cases come round; want = oracle.multi_miller_loop on the plain points, on first use"""
    a, b = C.g1_cases(oracle, pyref), C.g2_cases(oracle, pyref)
    g1s = [v for _, v in a.values()]
    keys = [v for _, v in b.values()]
    valid = [k for k, (cls, _) in enumerate(b.values()) if cls == "subgroup"]
    made = {}

    def get(n):
        if n not in made:
            idx = [valid[(i + i // len(g1s)) % len(valid)] for i in range(n)]
            g1 = b"".join(g1s[i % len(g1s)] for i in range(n))
            made[n] = (g1, np.array(idx, dtype=np.uint32), oracle.multi_miller_loop(g1, b"".join(keys[k] for k in idx), n))
        return made[n]
    return get


@pytest.mark.parametrize("name", ["default", "serial_prep"])
def test_key_preparation_on_every_named_key(engines, oracle, pyref, name):
    """g2_prepare_batch over all named G2 cases, four lanes per key and one lane per key: valid exactly for the subgroup class,
    which is the oracle's check with the identities cleared"""
    b = C.g2_cases(oracle, pyref)
    e = engines[name]
    keys = b"".join(v for _, v in b.values())
    prep, ran = launches(e, lambda: e.g2_prepare_batch(keys, len(b)), PREP_KERNELS)
    try:
        assert ran == {"g2_prepare": 1, "g2_expand": 1}
        got = bits_of(prep.valid_bitmap(), len(b))
    finally:
        prep.close()
    chk = bits_of(oracle.g2_check_batch(keys, len(b)), len(b))
    for (label, (cls, _)), bit, ok in zip(b.items(), got, chk):
        assert bit == (cls == "subgroup"), label
        assert bit == (ok and cls != "identity"), label


@pytest.mark.parametrize("name,n", [(name, n) for name in ("default", "serial_prep") for n in (1, 2, 3, 2048, 2049, 2050)])
def test_prepared_key_forms_on_every_g1_case(engines, prepared_terms, oracle, pyref, M, name, n):
    """multi_miller_loop_prepared: one wave per pair up to 2048 pairs (miller_wide_1p), then two pairs per lane (miller_hpk2p) with
    an odd and an even count, so the last lane is once half padding and once full; an index that names an invalid key is refused"""
    b = C.g2_cases(oracle, pyref)
    e = engines[name]
    g1, idx, want = prepared_terms(n)
    prep = e.g2_prepare_batch(b"".join(v for _, v in b.values()), len(b))
    try:
        got, ran = launches(e, lambda: e.multi_miller_loop_prepared(prep, idx, g1, n), MILLER_KERNELS)
        assert ran == {prepared_form(n): 1}
        assert got == want
        bad = idx.copy()
        bad[n - 1] = list(b).index("outside_0")
        with pytest.raises(M.InvalidG2Bytes):
            e.multi_miller_loop_prepared(prep, bad, g1, n)
        assert e.multi_miller_loop_prepared(prep, idx, g1, n) == want             # the context is usable afterwards
    finally:
        prep.close()


# ---------------- the verify path
@pytest.fixture(scope="module")
def vtable(oracle, pyref, M):
    return C.verify_table(oracle, pyref, M.DEFAULT_DST)


@pytest.mark.parametrize("name,size", [("default", s) for s in (1, 65, 2048, 2049, "tri_max", "tri_max + 1")] +
                         [(name, n) for name in ("tri", "lane") for n in (65, 300)])
def test_verify_forms_on_the_verify_table(engines, vtable, cus, name, size):
    """verify_batch over the tiled table (honest tuples under five keys of known secret key, -G2gen among them; every named G1 case,
    the identity and off-curve points as signatures; keys outside the r-torsion, off the twist and the identity): the oracle's
    bits, by the table-only Miller loop in the form the size dictates and, with the key preparation off, by the per-tuple loop.
    On the lane engine the sizes below 1024 take the per-tuple loop either way, as verify_chunk_dev says."""
    kinds, pks, msgs, sigs, bits = vtable
    n = size_of(size, cus)
    e = engines[name]
    v = C.spread(n)
    pk, sg, ms = C.tile(pks, n), C.tile(sigs, n), [msgs[i] for i in v]
    want = synth.bitmap_of([bits[i] for i in v])
    assert 2 * len(set(pks)) <= n or n <= cus * 64                        # few distinct keys: verify_chunk_dev prepares them

    def check(auto_prepare):
        got, ran = launches(e, lambda: e.verify_batch(pk, ms, sg), MILLER_KERNELS)
        assert ran == {verify_form(name, n, cus, auto_prepare): 1}
        if got != want:
            bad = [i for i in range(n) if bits_of(got, n)[i] != bits[v[i]]]
            raise AssertionError("n = %d: %d bits differ from the oracle, the first at %s" % (n, len(bad), [(i, int(v[i]), kinds[v[i]]) for i in bad[:8]]))
    check(True)
    e.set_auto_prepare(False)
    try:
        check(False)
    finally:
        e.set_auto_prepare(True)
