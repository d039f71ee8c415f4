"""The fixtures of the GPU tests.  A test module imports them by name; each stays module-scoped, so every module still gets an
engine (a context) of its own, closed when the module is done."""
import os

import pytest

from tests.library_support import M  # noqa: F401 (a fixture, imported from here by the GPU tests)


@pytest.fixture(scope="module")
def eng(M):
    e = M.Engine(0)           # raises when the HIP extension or the GPU is missing: no fallback
    yield e
    e.close()


def fresh_engine(M, monkeypatch, chunk, knobs=None):
    """an engine created under BLSBN254_CHUNK_LANES = chunk and the further BLSBN254_* settings of `knobs` (name -> string);
    the environment is as it was once the engine exists"""
    with monkeypatch.context() as mp:
        if chunk:
            mp.setenv("BLSBN254_CHUNK_LANES", chunk)
        for name, value in (knobs or {}).items():
            mp.setenv(name, value)
        return M.Engine(0)


# what selects the device form of the final exponentiation at a given size (run_final_exp, host.hip)
FE_FORM_KNOBS = ("BLSBN254_WIDE_FE", "BLSBN254_WIDE_FE_MAX", "BLSBN254_TRI_MAX", "BLSBN254_TRI_FE", "BLSBN254_SPLIT_EASY", "BLSBN254_CHUNK_LANES")
FE_KERNELS = ("fe_easy", "fe_easy_head", "fe_inv4", "fe_easy_tail", "fe_hard_wide", "fe_tri_hard", "fe_expx_h1", "fe_expx_h2", "fe_expx", "fe_h3")


# ... and of the Miller loop and of the key preparation (miller_to_ws, host.hip; launch_g2_prepare, launch_miller_prepared and
# verify_chunk_dev, host_verify.hip; launch_miller_raw, host_aggregate.hip): the same sizes, and three switches of their own
MILLER_FORM_KNOBS = FE_FORM_KNOBS + ("BLSBN254_TRI_MILLER", "BLSBN254_QUAD_PREP", "BLSBN254_AUTO_PREPARE")
# every Miller-loop kernel the host code launches, under the name its launch is recorded by
MILLER_KERNELS = ("miller_wide_1", "miller_tri_1", "miller_1", "miller_wide_1p", "miller_tri_1p", "miller_hpk1p", "miller_hpk2p", "miller_hpk2", "miller_hpk2r",
                  "miller_hpk", "miller_wide_prepared", "miller_tri_prepared", "miller_prepared", "miller_verify")
PREP_KERNELS = ("g2_prepare", "g2_expand")          # g2_prepare: k_g2_prepare_quad or k_g2_prepare, one name for both


def fe_forms_set_by_environment():
    """the names among FE_FORM_KNOBS that the environment sets: with any of them the sizes at which a form runs are not the
    production ones"""
    return [k for k in FE_FORM_KNOBS if k in os.environ]


def miller_forms_set_by_environment():
    """the same for MILLER_FORM_KNOBS"""
    return [k for k in MILLER_FORM_KNOBS if k in os.environ]


ENGINES = ("default", "tri", "lane")


@pytest.fixture(scope="module")
def engines(M, eng):
    """default: the production choice by size; tri: no wave-per-pair kernels; lane: neither those nor the quad ones; serial_prep:
    the key preparation on one lane per key"""
    if miller_forms_set_by_environment():
        pytest.skip("the environment sets %s: the forms do not run at their production sizes" % ", ".join(miller_forms_set_by_environment()))
    mp = pytest.MonkeyPatch()
    made = {"default": eng}
    try:
        made["tri"] = fresh_engine(M, mp, None, {"BLSBN254_WIDE_FE": "0"})
        made["lane"] = fresh_engine(M, mp, None, {"BLSBN254_WIDE_FE": "0", "BLSBN254_TRI_MAX": "0"})
        made["serial_prep"] = fresh_engine(M, mp, None, {"BLSBN254_QUAD_PREP": "0"})
        yield made
    finally:
        for name in ("tri", "lane", "serial_prep"):
            if name in made:
                made[name].close()


def launches(e, call, kernels):
    """call() with the engine's launch record on: (its result, {kernel name: launches} of those of `kernels` that ran, absent
    ones left out).  The record is switched off again whether call() returns or raises."""
    e.profile_enable(True); e.profile_reset()
    try:
        out = call()
        rec = e.profile_read()
    finally:
        e.profile_enable(False); e.profile_reset()
    return out, {k: rec[k]["launches"] for k in kernels if k in rec and rec[k]["launches"]}


def fe_launches(e, call):
    """launches() of the final-exponentiation kernels"""
    return launches(e, call, FE_KERNELS)


def fe_form(easy, hard):
    """the launch record of one final exponentiation: easy in ("one", "split"), hard in ("wide", "tri", "lane")"""
    names = {"one": ("fe_easy",), "split": ("fe_easy_head", "fe_inv4", "fe_easy_tail")}[easy]
    names += {"wide": ("fe_hard_wide",), "tri": ("fe_tri_hard",), "lane": ("fe_expx_h1", "fe_expx_h2", "fe_expx", "fe_h3")}[hard]
    return {k: 1 for k in names}
