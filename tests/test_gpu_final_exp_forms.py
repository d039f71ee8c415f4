"""GPU tests (MI355X) of the calls that take an Fp12 value from the caller -- final_exponentiation, aggregate_finish, gt_mul_batch,
gt_pow_batch -- on ARBITRARY canonical inputs (tests/fp12_cases.py: zero, subfield elements, monomials, limb-boundary coefficients,
plain random values, tiled without a period), byte for byte against the oracle.  Every assertion about a device form of the final
exponentiation (run_final_exp, host.hip) also asserts, from the engine's launch record, that this form ran and no other."""
import random

import numpy as np
import pytest

from tests import fp12_cases as F
from tests import synth
from tests.gpu_support import eng, fe_form, fe_forms_set_by_environment, fe_launches, fresh_engine, M
from tests.helpers import b32

pytestmark = pytest.mark.gpu
ENGINES = ("default", "tri", "lane")
WIDE_MAX = 2048                                   # wide_fe_max of host_common.h


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def engines(M, eng):
    """default: the production choice by size; tri: no wave-per-tuple kernels; lane: neither those nor the three-lane ones"""
    if fe_forms_set_by_environment():
        pytest.skip("the environment sets %s: the forms do not run at their production sizes" % ", ".join(fe_forms_set_by_environment()))
    mp = pytest.MonkeyPatch()
    made = {"default": eng}
    try:
        made["tri"] = fresh_engine(M, mp, None, {"BLSBN254_WIDE_FE": "0"})
        made["lane"] = fresh_engine(M, mp, None, {"BLSBN254_WIDE_FE": "0", "BLSBN254_TRI_MAX": "0"})
        yield made
    finally:
        for name in ("tri", "lane"):
            if name in made:
                made[name].close()


@pytest.fixture(scope="module")
def cases(oracle, pyref):
    return F.values(oracle, pyref)


def hard_form(name, n, cus):
    """which hard part run_final_exp takes for a launch of n tuples on that engine"""
    if name == "default" and n <= WIDE_MAX:
        return "wide"
    return "tri" if name != "lane" and n <= cus * 64 else "lane"


def check_tiled_final_exp(e, cases, n, want_form, roll=0):
    names, vals, fes = cases
    assert all(count < 0.02 * n for count in F.repeats(n).values())       # the input condition, for the sizes this device gives
    data, want = F.tile(vals, n, roll=roll), F.tile(fes, n, roll=roll)
    got, ran = fe_launches(e, lambda: e.final_exponentiation(data, n))
    assert ran == want_form
    if got != want:
        v = np.roll(F.spread(n), roll)
        bad = [i for i in range(n) if got[384 * i:384 * i + 384] != want[384 * i:384 * i + 384]]
        raise AssertionError("n = %d: %d values differ from the oracle, the first at %s" % (n, len(bad), [(i, int(v[i]), names[v[i]]) for i in bad[:8]]))
    return got


@pytest.mark.parametrize("name,size", [(name, n) for name in ENGINES for n in (1, 63, 64, 65, 251, 2048)] +
                         [("default", s) for s in (2049, "tri_max", "tri_max + 1")])
def test_hard_part_forms_on_arbitrary_values(engines, cases, cus, name, size):
    """one tuple, a partial and a full 64-tuple workgroup of the three-lane grid, a second workgroup, every value of the tile, and
    each production switch-over from both sides (2048 | 2049: wave per tuple | three lanes; tri_max | tri_max + 1: three lanes | one
    lane per tuple)"""
    n = size if isinstance(size, int) else cus * 64 + (size == "tri_max + 1")
    e = engines[name]
    check_tiled_final_exp(e, cases, n, fe_form("one", hard_form(name, n, cus)))
    if n == 1:                                        # the tile's first position is the zero case: a plain random value alone too
        names, vals, fes = cases
        got, ran = fe_launches(e, lambda: e.final_exponentiation(vals[F.N_NAMED], 1))
        assert ran == fe_form("one", hard_form(name, 1, cus)) and got == fes[F.N_NAMED]


@pytest.mark.parametrize("k", [-1, 0, 1, 2, 3])
def test_split_easy_part_ragged_quarters(engines, cases, cus, k):
    """n = T - 1 runs k_fe_easy; from T = CUs x 128 on, k_fe_inv4 shares one Fp inversion among the tuples j, j + q, j + 2q, j + 3q
    (q = ceil(n / 4)): all four residues of n mod 4, so the last lanes' fourth tuple is past the end for three of them; zeros at
    the first position, at q - 1 and at n - 1 stay zero and leave the values they share an inversion with alone."""
    names, vals, fes = cases
    n = cus * 128 + k
    got = check_tiled_final_exp(engines["default"], cases, n, fe_form("one" if k < 0 else "split", "lane"))
    v = F.spread(n)
    for z in F.zero_positions(n):
        assert got[384 * z:384 * z + 384] == F.ZERO_GT, z
        ps = F.partners(n, z)
        assert len(ps) >= 2
        for p in ps:
            assert v[p] >= F.N_NAMED and got[384 * p:384 * p + 384] == fes[v[p]] and fes[v[p]] not in (F.ZERO_GT, F.ONE_GT), (z, p)
    # the same values one position up: the last tuple (alone in its quarter when n % 4 == 1) and the lanes' fourth tuples are then
    # plain values, whose result shows whether their inversion was taken at all, which the zero's does not
    check_tiled_final_exp(engines["default"], cases, n, fe_form("one" if k < 0 else "split", "lane"), roll=1)


@pytest.fixture(scope="module")
def finish_cases(eng, oracle, pyref, cases, M):
    """[(label, partials, k)] for aggregate_finish(partials, k, None); the honest partial carries ML(agg_sig, -G2gen)"""
    names, vals, fes = cases
    val = lambda name: vals[names.index(name)]
    x, xi = F.inverse_pair(oracle, pyref)
    dst = M.DEFAULT_DST
    n = 5
    sks = [synth.sk_of(300 + k) for k in range(n)]
    pks = b"".join(oracle.sk_to_pk(s) for s in sks)
    msgs = [synth.msg_of(300 + i) for i in range(n)]
    agg = oracle.aggregate_sigs(b"".join(oracle.sign(s, m, dst) for s, m in zip(sks, msgs)), n)
    neg_g2 = pyref.g2_to_bytes(pyref.g2_neg(pyref.G2_GEN))
    out = [("fp6 alone", val("fp6"), 1), ("w fp6 alone", val("w_fp6"), 1), ("x and 1/x", x + xi, 2), ("random alone", x, 1),
           ("zero", val("zero"), 1), ("x and zero", x + val("zero"), 2)]
    for label, ms in (("honest", msgs), ("tampered", msgs[:3] + [b"tampered"] + msgs[4:])):
        part, ok, sok = eng.aggregate_partial_with_sig(pks, ms, agg, dst)
        assert ok and sok and part == oracle.multi_miller_loop(oracle.hash_to_g1_batch(ms, dst) + agg, pks + neg_g2, n + 1)
        out.append((label + " partial", part, 1))
        out.append((label + " partial times an Fp6 element", part + val("fp6"), 2))
    return out


@pytest.mark.parametrize("name", ENGINES)
def test_single_flag_mode_on_arbitrary_partials(engines, finish_cases, oracle, cus, name):
    """aggregate_finish(partials, k, NULL): the product of caller-supplied partials through mode 3 of each hard part (the lane
    engine is the only route to k_fe_h3's); the expectation is the oracle's final exponentiation of the oracle's product"""
    e = engines[name]
    verdict = {}
    for label, partials, k in finish_cases:
        prod = F.ONE_GT
        for j in range(k):
            prod = oracle.gt_mul(prod, partials[384 * j:384 * j + 384])
        want = oracle.final_exponentiation(prod, 1) == F.ONE_GT
        got, ran = fe_launches(e, lambda: e.aggregate_finish(partials, k, None))
        assert ran == fe_form("one", hard_form(name, 1, cus)), label
        assert got is want, label
        verdict[label] = got
    assert verdict["fp6 alone"] and verdict["w fp6 alone"] and verdict["x and 1/x"] and not verdict["random alone"] and not verdict["zero"]
    assert verdict["honest partial"] is True and verdict["honest partial times an Fp6 element"] is verdict["honest partial"]
    assert verdict["tampered partial"] is False and verdict["tampered partial times an Fp6 element"] is False


MUL_PARTNER = lambda v: (13 * v + 5) % F.D          # the second operand's value index: a bijection of the first's
N_SCALARS = 37                                      # value v is raised to scalar v % 37: the six edge scalars meet named and random values


@pytest.fixture(scope="module")
def gt_refs(oracle, pyref, cases):
    """per value of the tile: its partner in the product and its scalar, with the oracle's gt_mul and gt_pow of each, computed once
    for all sizes (the oracle takes about 4 ms per power)"""
    names, vals, fes = cases
    rnd = random.Random(0x6710)
    ks = [0, 1, 2, pyref.R - 1, pyref.R, (1 << 256) - 1] + [rnd.randrange(1 << 256) for _ in range(N_SCALARS - 6)]
    partner = [vals[MUL_PARTNER(v)] for v in range(F.D)]
    scalar = [b32(ks[v % N_SCALARS]) for v in range(F.D)]
    return {"partner": partner, "scalar": scalar, "mul": [oracle.gt_mul(vals[v], partner[v]) for v in range(F.D)],
            "pow": [oracle.gt_pow(vals[v], scalar[v]) for v in range(F.D)]}


@pytest.mark.parametrize("n", [255, 256, 257, 1000])
def test_gt_mul_pow_beyond_one_workgroup_and_outside_gt(eng, cases, gt_refs, n):
    """gt_mul_batch / gt_pow_batch over the tiled arbitrary values (zero and non-cyclotomic elements included: k_gt_pow squares
    generically) with scalars 0, 1, 2, r - 1, r, 2^256 - 1 and random 256-bit ones: a workgroup of 256 lanes less one, exactly one,
    one more, and several; per element against the oracle's gt_mul / gt_pow"""
    names, vals, fes = cases
    v = [int(x) for x in F.spread(n)]
    a = F.tile(vals, n)
    got_mul = eng.gt_mul_batch(a, F.tile(gt_refs["partner"], n), n)
    got_pow = eng.gt_pow_batch(a, F.tile(gt_refs["scalar"], n), n)
    for i in range(n):
        assert got_mul[384 * i:384 * i + 384] == gt_refs["mul"][v[i]], ("gt_mul", i, names[v[i]], names[MUL_PARTNER(v[i])])
        assert got_pow[384 * i:384 * i + 384] == gt_refs["pow"][v[i]], ("gt_pow", i, names[v[i]], gt_refs["scalar"][v[i]].hex())


def test_gt_batches_reject_a_non_canonical_coefficient_mid_batch(eng, cases, pyref, M):
    names, vals, fes = cases
    n = 1000
    a = F.tile(vals, n)
    bad = bytearray(a)
    bad[384 * 500 + 32 * 7:384 * 500 + 32 * 8] = b32(pyref.P)          # element 500, coefficient 7: p itself
    bad = bytes(bad)
    ks = b32(3) * n
    with pytest.raises(M.InvalidGtBytes):
        eng.gt_mul_batch(bad, a, n)
    with pytest.raises(M.InvalidGtBytes):
        eng.gt_mul_batch(a, bad, n)
    with pytest.raises(M.InvalidGtBytes):
        eng.gt_pow_batch(bad, ks, n)
    with pytest.raises(M.InvalidGtBytes):
        eng.final_exponentiation(bad, n)
    assert eng.gt_pow_batch(a[:384 * 3], b32(1) * 3, 3) == a[:384 * 3]   # the context is usable afterwards
