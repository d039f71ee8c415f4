"""CPU-only: the arbitrary Fp12 inputs of tests/fp12_cases.py.  The tiling has no period at the distances at which a kernel could
read a neighbour's value and places its zeros where k_fe_inv4 shares an inversion; the oracle's final exponentiation equals the
independent pure-Python model outside the image of the Miller loop; the device headers compiled for the host (serial, wave-per-
tuple and three-lane hard part) equal the oracle on every named case."""
import ctypes

import pytest

from tests import fp12_cases as F
from tests import hostsim_build


@pytest.fixture(scope="module")
def hs():
    return ctypes.CDLL(hostsim_build.build("hostsim.cpp", "libhostsim.so"))


def test_named_cases_are_canonical_and_repeatable(oracle, pyref):
    a, b = F.named_cases(oracle, pyref), F.named_cases(oracle, pyref)
    assert list(a.items()) == list(b.items()) and len(set(a.values())) == len(a) == F.N_NAMED
    for name, v in a.items():
        assert pyref.f12_from_bytes(v) is not None, name            # every coefficient below p
    names, vals, fes = F.values(oracle, pyref)
    assert names[:F.N_NAMED] == list(a) and vals[:F.N_NAMED] == list(a.values()) and names[F.N_NAMED:] == [None] * (F.D - F.N_NAMED)
    assert len(set(vals)) == F.D and all(pyref.f12_from_bytes(v) is not None for v in vals)
    assert fes[names.index("zero")] == F.ZERO_GT                    # inv0: 0 -> 0
    for name in F.SUBFIELD:
        assert fes[names.index(name)] == F.ONE_GT, name             # proper subfields -> the identity
    for i in range(F.N_NAMED, F.D):
        assert fes[i] not in (F.ZERO_GT, F.ONE_GT)
    x, xi = F.inverse_pair(oracle, pyref)
    assert xi == a["inverse"] and oracle.gt_mul(x, xi) == F.ONE_GT


# 256 compute units is the MI355X; the others stand for a partitioned device: the sizes around tri_max and the split-easy
# threshold follow the count (the GPU tests check the same conditions again for the count they find)
@pytest.mark.parametrize("cus", [256, 128, 64, 32])
def test_spread_has_no_period_and_places_the_zeros(cus):
    for n in F.sizes(cus):
        v = F.spread(n)
        assert len(v) == n and v.min() >= 0 and v.max() < F.D
        for dist, count in F.repeats(n).items():
            assert count < 0.02 * n, (n, dist, count)
        q = (n + 3) // 4
        zs = F.zero_positions(n)
        assert {0, q - 1, n - 1} == set(zs) and all(v[z] == F.ZERO for z in zs)
        for z in zs:
            ps = F.partners(n, z)
            assert set(ps) == {z + k * q for k in range(-3, 4) if k and 0 <= z + k * q < n} - set(zs)
            assert all(v[p] >= F.N_NAMED for p in ps), (n, z)                     # plain random: not zero, in no subfield
        if n >= 2 * F.D:
            assert len(set(v.tolist())) == F.D                                    # every value is in the batch


def test_oracle_final_exponentiation_equals_python_model(oracle, pyref):
    """the reference itself outside Miller values: the C oracle against the structurally different pure-Python model (slow: a
    small subset)"""
    names, vals, fes = F.values(oracle, pyref)
    for name in ("zero", "minus_one", "fp2", "w_fp6", "all_p_minus_1", "hole_3", "edges"):
        i = names.index(name)
        assert pyref.f12_to_bytes(pyref.final_exponentiation(pyref.f12_from_bytes(vals[i]))) == fes[i], name


def test_host_forms_equal_oracle_on_named_cases(hs, oracle, pyref):
    """the device headers on the host: the serial final exponentiation, the wave-per-tuple hard part (wide.h) and the three-lane
    hard part (tri.h, with its per-lane comparison with one) against the oracle on every named case and a few random values"""
    names, vals, fes = F.values(oracle, pyref)
    out = ctypes.create_string_buffer(384)
    one = ctypes.c_int(-1)
    for i in list(range(F.N_NAMED)) + [F.N_NAMED, F.N_NAMED + 1, F.D - 1]:
        assert hs.hs_final_exp(vals[i], out) == 0 and out.raw == fes[i], names[i]
        assert hs.hs_final_exp_wide(vals[i], out) == 0 and out.raw == fes[i], names[i]
        assert hs.hs_tri_final_exp(vals[i], out, ctypes.byref(one)) == 0 and out.raw == fes[i], names[i]
        assert one.value == int(fes[i] == F.ONE_GT), names[i]
