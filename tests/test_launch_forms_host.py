"""CPU-only: which device form runs at which size (bls-bn254_amd/csrc/launch_forms.h, the very header the host units compile):
the settings and their environment overrides, and one function per decision -- the hard and the easy part of the final
exponentiation, the variable-point and the table-only Miller loops, two pairs per lane, the key preparation, "small enough for
the prepared path" and the gate of the grouped aggregate verify -- driven through the stand-alone program
tests/hostsim/launch_forms_host.cpp and compared with a model written here from the prose of DESIGN.md ("Launch forms").  The
program is built twice -- plain, and with -fsanitize=address,undefined -fno-sanitize-recover -- and both are run as ordinary
programs.  A test tool; the product has no CPU path."""
import itertools
import re
import subprocess

import pytest

from tests import hostsim_build

MR_WIDE, MR_TRI, MR_ONE, MR_TWO, MR_ALL = 1, 2, 4, 8, 15
# the admitted forms the call sites of launch_miller_raw pass: the sharded / prepared aggregate calls, the grouped aggregate verify
# and round 1 of the aggregate RLC, the Miller product over prepared keys, the later rounds of the aggregate RLC
SITE_MASKS = (MR_TWO, MR_ALL, MR_WIDE | MR_TWO, MR_ALL & ~MR_TWO)
CHUNK = 1 << 22             # blsbn254_ctx::chunk
FIELDS = ("lanes", "wide", "wide_max", "tri_max", "tri_miller", "tri_fe", "split_easy", "quad_prep")
DEFAULTS = dict(lanes=65536, wide=1, wide_max=2048, tri_max=16384, tri_miller=1, tri_fe=1, split_easy=1, quad_prep=1)
SWITCHES = ("wide", "tri_miller", "tri_fe", "split_easy", "quad_prep")
SETTINGS = ([DEFAULTS] + [dict(DEFAULTS, **{s: 0}) for s in SWITCHES] +
            [dict(DEFAULTS, wide_max=0), dict(DEFAULTS, tri_max=0), dict(DEFAULTS, tri_max=1000), dict(DEFAULTS, lanes=304 * 256, tri_max=304 * 64)])


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def prog(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("launch_forms_" + request.param) / "launch_forms_host"
    return hostsim_build.build("launch_forms_host.cpp", exe, shared=False, extra=hostsim_build.SANITIZED if request.param == "sanitized" else ())


def run(prog, tmp_path, lines):
    """one command per line -> the words behind the command's name, per line"""
    script = tmp_path / "commands.txt"
    script.write_text("".join(" ".join(str(x) for x in ln) + "\n" for ln in lines))
    out = subprocess.run([prog, str(script)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    got = [ln.split() for ln in out.stdout.splitlines()]
    assert [g[0] for g in got] == [ln[0] for ln in lines]
    return [g[1:] for g in got]


def words(S):
    return tuple(S[f] for f in FIELDS)


# ------------------------------------------------------------------ the model
def fe_hard(S, n):
    if S["wide"] and n <= S["wide_max"]:
        return "wide"
    return "tri" if S["tri_fe"] and n <= S["tri_max"] else "lane"


def fe_split(S, n):
    return bool(S["split_easy"]) and n >= S["lanes"] // 2


def miller(S, n):
    if S["wide"] and n <= S["wide_max"] // 2:
        return "wide"
    return "tri" if S["tri_miller"] and n <= S["tri_max"] else "lane"


def table(S, n, mask):
    if mask & MR_WIDE and S["wide"] and n <= S["wide_max"]:
        return "wide"
    return "tri" if mask & MR_TRI and S["tri_miller"] and n <= S["tri_max"] else "lane"


def two(S, n, mask, chunk):
    """two pairs per lane: no small form takes the launch, and one pair per lane (a launch within half a round of lanes, a site
    that does not admit two, a launch beyond the chunk) does not either"""
    if table(S, n, mask) != "lane":
        return False
    one = bool(mask & MR_ONE) and (2 * n <= S["lanes"] or not mask & MR_TWO or n > chunk)
    return not one


def prep(S, u):
    return bool(S["quad_prep"]) and 8 * u <= S["lanes"]


def small(S, n, per_tuple_fe):
    by_wave = S["wide"] and n <= S["wide_max"]
    by_quad = S["tri_miller"] and (S["tri_fe"] or not per_tuple_fe) and n <= S["tri_max"]
    return bool(by_wave or by_quad)


def grouped(S, n):
    return bool(S["wide"]) and n <= S["wide_max"]


def atoi(text):
    m = re.match(r"\s*([+-]?\d+)", text)
    return int(m.group(1)) if m else 0


def from_env(env, cus):
    S = dict(DEFAULTS, lanes=cus * 256, tri_max=cus * 256 // 4)
    for name, field in (("BLSBN254_WIDE_FE", "wide"), ("BLSBN254_QUAD_PREP", "quad_prep"), ("BLSBN254_SPLIT_EASY", "split_easy"),
                        ("BLSBN254_TRI_MILLER", "tri_miller"), ("BLSBN254_TRI_FE", "tri_fe")):
        if name in env:
            S[field] = int(atoi(env[name]) != 0)
    for name, field in (("BLSBN254_TRI_MAX", "tri_max"), ("BLSBN254_WIDE_FE_MAX", "wide_max")):
        if name in env and 0 <= atoi(env[name]) <= 1 << 20:
            S[field] = atoi(env[name])
    return S


def grid(S, chunk):
    limits = (S["wide_max"] // 2, S["wide_max"], S["tri_max"], S["lanes"] // 8, S["lanes"] // 4, S["lanes"] // 2, chunk)
    return sorted({0, 1} | {max(L + d, 0) for L in limits for d in (-1, 0, 1)})


def yes(b):
    return [str(int(b))]


# ------------------------------------------------------------------ the tests
def test_defaults_and_the_documented_switch_overs(prog, tmp_path):
    D = DEFAULTS
    cmds = [("defaults",)]
    cmds += [("fe_hard",) + words(D) + (n,) for n in (2048, 2049, 16384, 16385)]
    cmds += [("miller",) + words(D) + (n,) for n in (1024, 1025, 16384, 16385)]
    cmds += [("fe_split",) + words(D) + (n,) for n in (32767, 32768)]
    cmds += [("prep",) + words(D) + (u,) for u in (8192, 8193)]
    cmds += [("two",) + words(D) + (n, MR_ALL, CHUNK) for n in (16385, 32768, 32769)]
    cmds += [("two",) + words(D) + (1, MR_TWO, CHUNK), ("two",) + words(D) + (2049, MR_WIDE | MR_TWO, CHUNK), ("two",) + words(D) + (1 << 20, MR_ALL & ~MR_TWO, CHUNK)]
    cmds += [("grouped",) + words(D) + (n,) for n in (2048, 2049)]
    cmds += [("small",) + words(dict(D, tri_fe=0)) + (2049, fe) for fe in (1, 0)]
    want = [[str(x) for x in words(D)]]
    want += [["wide"], ["tri"], ["tri"], ["lane"]] * 2
    want += [["0"], ["1"]] + [["1"], ["0"]] + [["0"], ["0"], ["1"]] + [["1"], ["1"], ["0"]] + [["1"], ["0"]] + [["0"], ["1"]]
    assert run(prog, tmp_path, cmds) == want


@pytest.mark.parametrize("k", range(len(SETTINGS)))
def test_every_rule_around_every_limit(prog, tmp_path, k):
    S = SETTINGS[k]
    cmds, want = [], []
    for chunk in (CHUNK, 64):
        for n in grid(S, chunk):
            w = words(S)
            cmds += [("fe_hard",) + w + (n,), ("fe_split",) + w + (n,), ("miller",) + w + (n,), ("prep",) + w + (n,), ("grouped",) + w + (n,)]
            want += [[fe_hard(S, n)], yes(fe_split(S, n)), [miller(S, n)], yes(prep(S, n)), yes(grouped(S, n))]
            for fe in (0, 1):
                cmds.append(("small",) + w + (n, fe)); want.append(yes(small(S, n, fe)))
            for mask in SITE_MASKS:
                cmds.append(("table",) + w + (n, mask)); want.append([table(S, n, mask)])
                cmds.append(("two",) + w + (n, mask, chunk)); want.append(yes(two(S, n, mask, chunk)))
    assert run(prog, tmp_path, cmds) == want


def test_the_loop_and_the_exponentiation_behind_it_agree(prog, tmp_path):
    """a verify launch's Miller loop and final exponentiation are both asked with the same n: with both quad halves on they name
    the same form at every size, and the prepared path is taken for exactly the sizes at which one of them is not a lane"""
    cmds = []
    for S in SETTINGS:
        for n in grid(S, CHUNK):
            cmds += [("table",) + words(S) + (n, MR_ALL), ("fe_hard",) + words(S) + (n,), ("small",) + words(S) + (n, 1)]
    got = run(prog, tmp_path, cmds)
    i = 0
    for S in SETTINGS:
        for n in grid(S, CHUNK):
            ml, fe, sm = got[i][0], got[i + 1][0], got[i + 2][0]
            i += 3
            if S["tri_miller"] and S["tri_fe"]:
                assert ml == fe, (S, n)
                assert (sm == "1") == (ml != "lane"), (S, n)
            if sm == "1":
                assert ml != "lane", (S, n)


VARS = ("BLSBN254_WIDE_FE", "BLSBN254_QUAD_PREP", "BLSBN254_SPLIT_EASY", "BLSBN254_TRI_MILLER", "BLSBN254_TRI_FE", "BLSBN254_TRI_MAX", "BLSBN254_WIDE_FE_MAX")


def test_settings_from_the_environment(prog, tmp_path):
    envs = [{}]
    envs += [{v: x} for v in VARS for x in ("0", "1", "abc", "7x", "-1")]
    envs += [{v: x} for v in VARS[5:] for x in (str(1 << 20), str((1 << 20) + 1), "99999999999")]
    envs += [dict(zip(VARS, xs)) for xs in itertools.product(("0", "2"), repeat=len(VARS))][::9]
    cmds, want = [], []
    for cus in (1, 256, 304):
        for env in envs:
            cmds.append(("env", cus, len(env)) + tuple(x for kv in env.items() for x in kv))
            want.append([str(x) for x in words(from_env(env, cus))])
    got = run(prog, tmp_path, cmds)
    assert got == want
    by = {(c[1], c[3:]): g for c, g in zip(cmds, got)}
    t = FIELDS.index("tri_max")
    assert by[(304, ())][t] == str(304 * 64) and by[(304, ("BLSBN254_TRI_MAX", "1"))][t] == "1"          # the override wins over the derived limit
    assert by[(256, ("BLSBN254_TRI_MAX", str((1 << 20) + 1)))][t] == "16384" and by[(256, ("BLSBN254_TRI_MAX", "-1"))][t] == "16384"
    assert by[(256, ("BLSBN254_TRI_MAX", "abc"))][t] == "0"                                               # atol of a non-number: 0, in range
    assert by[(256, ())] == [str(x) for x in words(DEFAULTS)]
