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


def fe_forms_set_by_environment():
    """the names among FE_FORM_KNOBS that the environment sets: with any of them the sizes at which a form runs are not the
    production ones"""
    return [k for k in FE_FORM_KNOBS if k in os.environ]


def fe_launches(e, call):
    """call() with the engine's launch record on: (its result, {kernel name: launches} of the final-exponentiation kernels that
    ran, absent ones left out)"""
    e.profile_enable(True); e.profile_reset()
    try:
        out = call()
        rec = e.profile_read()
    finally:
        e.profile_enable(False); e.profile_reset()
    return out, {k: rec[k]["launches"] for k in FE_KERNELS if k in rec and rec[k]["launches"]}


def fe_form(easy, hard):
    """the launch record of one final exponentiation: easy in ("one", "split"), hard in ("wide", "tri", "lane")"""
    names = {"one": ("fe_easy",), "split": ("fe_easy_head", "fe_inv4", "fe_easy_tail")}[easy]
    names += {"wide": ("fe_hard_wide",), "tri": ("fe_tri_hard",), "lane": ("fe_expx_h1", "fe_expx_h2", "fe_expx", "fe_h3")}[hard]
    return {k: 1 for k in names}
