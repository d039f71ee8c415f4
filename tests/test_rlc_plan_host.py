"""CPU-only: what the host decides without the device in the batch verification by random linear combination
(bls-bn254_amd/csrc/rlc_plan.h, the very header host_rlc.hip compiles): the "keys repeat" test, the chunk-size rule, the bounds
of the counts read back from the device and the back-off of the key round, driven through the stand-alone program
tests/hostsim/rlc_plan_host.cpp and compared with a model written here from the prose of DESIGN.md 5 ("The host side ... and
what it decides alone").  The program is built twice -- plain, and with -fsanitize=address,undefined -fno-sanitize-recover --
and both are run as ordinary programs.  A test tool; the product has no CPU path."""
import random
import subprocess

import pytest

from tests import hostsim_build

MAX_KEYS = 65536            # PREP_MAX_KEYS
R, TRI_MAX, WIDE_MAX = 65536, 16384, 2048       # an MI355X: 256 CUs x 256 lanes, a quarter of that, BLSBN254_WIDE_FE_MAX's default


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def prog(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("rlc_plan_" + request.param) / "rlc_plan_host"
    return hostsim_build.build("rlc_plan_host.cpp", exe, shared=False, extra=hostsim_build.SANITIZED if request.param == "sanitized" else ())


def run(prog, tmp_path, lines):
    """one command per line -> the words behind the command's name, per line"""
    script = tmp_path / "commands.txt"
    script.write_text("".join(" ".join(str(x) for x in ln) + "\n" for ln in lines))
    out = subprocess.run([prog, str(script)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    got = [ln.split() for ln in out.stdout.splitlines()]
    assert [g[0] for g in got] == [ln[0] for ln in lines]
    return [g[1:] for g in got]


# ------------------------------------------------------------------ the model
def keys_repeat(n, u):
    return 2 * u <= n and u <= MAX_KEYS


def bound(n, g, u):
    return n // g + u


def rounds(b, r):
    return -(-b // r)


def chunk_size(n, u, group=16, auto=True, r=R, tri=True, tri_max=TRI_MAX, wide_max=WIDE_MAX):
    if not auto:
        return group
    G = group
    if rounds(bound(n, G, u), r) > 1:                                   # rule 1: a whole round of waves saved
        better = [g for g in range(G + 1, 2 * G + 1) if rounds(bound(n, g, u), r) < rounds(bound(n, G, u), r)]
        G = better[0] if better else G
    if tri and tri_max > wide_max and bound(n, G, u) > tri_max:         # rule 2: under the limit of the three-lane kernels
        better = [g for g in range(G + 1, 2 * G + 1) if bound(n, g, u) <= tri_max]
        G = better[0] if better else G
    return G


class Backoff:
    def __init__(self):
        self.skip = self.streak = 0

    def call(self, enabled, passes):
        """-> was the key round taken"""
        if not enabled:
            return False
        if self.skip > 0:
            self.skip -= 1
            return False
        if passes:
            self.streak = 0
        else:
            self.streak = min(self.streak + 1, 4)
            self.skip = 2 ** self.streak
        return True


def model_backoff(ops):
    b, enabled, out = Backoff(), True, []
    for op in ops:
        if op == "R":
            b.skip = b.streak = 0
        elif op in "ED":
            enabled = op == "E"
        else:
            taken = b.call(enabled, op == "P")
            out.append("%d:%d:%d" % (taken, b.skip, b.streak))
    return out


def size_cmd(n, u, group=16, auto=True, r=R, tri=True, tri_max=TRI_MAX, wide_max=WIDE_MAX):
    return ("size", n, u, group, int(auto), r, int(tri), tri_max, wide_max)


# ------------------------------------------------------------------ the tests
def test_the_documented_chunk_size(prog, tmp_path):
    n, u = 262144, 1024
    assert (bound(n, 16, u), bound(n, 17, u), bound(n, 18, u)) == (17408, 16444, 15587)
    assert chunk_size(n, u) == 18                                       # rule 1 does not fire (one round), rule 2 does
    (got,) = run(prog, tmp_path, [size_cmd(n, u)])
    assert got == ["18", "15587"]


def test_an_explicit_group_is_not_searched(prog, tmp_path):
    # the sizes at which both rules would fire, and a group that is not the default
    cases = [(262144, 1024, 16), (1048576, 13, 16), (262144, 1024, 2), (5000, 7, 4096)]
    got = run(prog, tmp_path, [size_cmd(n, u, group=g, auto=False) for n, u, g in cases])
    assert got == [[str(g), str(bound(n, g, u))] for n, u, g in cases]


def test_tri_disabled(prog, tmp_path):
    n, u = 262144, 1024
    # the three-lane kernels off; their limit at or below the wave-per-tuple limit (BLSBN254_TRI_MAX=0 among them)
    cmds = [size_cmd(n, u, tri=False), size_cmd(n, u, tri_max=0), size_cmd(n, u, tri_max=2048), size_cmd(n, u, tri_max=2049)]
    got = run(prog, tmp_path, cmds)
    assert got[:3] == [["16", "17408"]] * 3
    # 2049 is above the wave-per-tuple limit: rule 2 looks, and no g up to 32 brings 262144 tuples under it
    assert chunk_size(n, u, tri_max=2049) == 16 and got[3] == ["16", "17408"]


def test_a_whole_round_of_waves_saved(prog, tmp_path):
    # 1 048 576 tuples over 13 keys: 65 549 chunks at G = 16 are 13 over one round of 65 536; 17 per chunk fit (61 693).  Rule 2
    # then finds no g up to 34 under 16 384.  Chosen with the model:
    n, u = 1048576, 13
    assert (bound(n, 16, u), rounds(bound(n, 16, u), R), bound(n, 17, u)) == (65549, 2, 61693) and chunk_size(n, u) == 17
    # and on a small device (R = 256, three-lane limit 64): 4100 tuples over 4 keys need 2 rounds at 16, 1 at 17
    small = dict(r=256, tri_max=64, wide_max=8)
    assert (bound(4100, 16, 4), bound(4100, 17, 4)) == (260, 245) and chunk_size(4100, 4, **small) == 17
    # both rules in one call: rule 1 leaves 17 (245 chunks > 200), rule 2 searches 18 .. 34 from there: 4100 // 21 + 4 = 199
    both = dict(r=256, tri_max=200, wide_max=8)
    assert chunk_size(4100, 4, **both) == 21
    got = run(prog, tmp_path, [size_cmd(n, u), size_cmd(4100, 4, **small), size_cmd(4100, 4, **both)])
    assert got == [["17", "61693"], ["17", "245"], ["21", "199"]]


def test_keys_repeat_at_the_boundary(prog, tmp_path):
    cases = [(2 * u, u) for u in (1, 2, 5, 1024, MAX_KEYS)] + [(2 * u - 1, u) for u in (1, 2, 5, 1024, MAX_KEYS)]
    cases += [(2 * (MAX_KEYS + 1), MAX_KEYS + 1), (1 << 22, MAX_KEYS), (1 << 22, MAX_KEYS + 1), (2, 2), (3, 1)]
    got = run(prog, tmp_path, [("repeat", n, u, MAX_KEYS) for n, u in cases])
    assert [g == ["1"] for g in got] == [keys_repeat(n, u) for n, u in cases]
    assert [g == ["1"] for g in got[:10]] == [True] * 5 + [False] * 5    # n = 2 u: taken; n = 2 u - 1: not


def test_bounds(prog, tmp_path):
    cmds, want = [], []
    for items, G, u in ((96, 16, 4), (200, 2, 2), (262144, 18, 1024), (100, 32, 2), (0, 32, 1), (31, 32, 5)):
        cmds.append(("bound", items, G, u)); want.append([str(items // G + u)])
    n, u, items = 96, 4, 40
    m_max = bound(items, 32, u)                                         # 5
    for m in (0, 1, n - 1, n, n + 1):
        cmds.append(("chunks", m, n)); want.append([str(int(1 <= m <= n))])
    for m in (0, u - 1, u, m_max, m_max + 1):
        cmds.append(("level", m, u, m_max, items)); want.append([str(int(u <= m <= m_max and m <= items))])
    cmds.append(("level", 4, 2, 9, 3)); want.append(["0"])              # inside the reserve, but more chunks than items
    cmds.append(("level", 3, 2, 9, 3)); want.append(["1"])
    for mc in (0, 1, 7, 8):
        cmds.append(("list", mc, 7)); want.append([str(int(1 <= mc <= 7))])
    for m2 in (0, 1, n, n + 1):
        cmds.append(("fallback", m2, n)); want.append([str(int(m2 <= n))])
    assert run(prog, tmp_path, cmds) == want


def test_the_back_off(prog, tmp_path):
    # a failure, then 2 calls pass through (what they would have been does not matter), a failure, 4, a failure, 8, a failure,
    # 16, a failure, 16 again (capped), a pass (taken: it resets), and the next failure starts at 2 again
    ops = "F" + "PF" + "F" + "PFPF" + "F" + "P" * 8 + "F" + "F" * 16 + "F" + "P" * 16 + "P" + "F" + "PP" + "P"
    (got,) = run(prog, tmp_path, [("backoff", ops)])
    assert got == model_backoff(ops)
    taken = [i for i, g in enumerate(got) if g.startswith("1:")]
    assert [b - a - 1 for a, b in zip(taken, taken[1:])] == [2, 4, 8, 16, 16, 0, 2]
    assert [got[i] for i in taken] == ["1:2:1", "1:4:2", "1:8:3", "1:16:4", "1:16:4", "1:0:0", "1:2:1", "1:0:0"]
    # reset clears a back-off in progress, the streak too: the call behind it takes the round, and a failure starts at 2 again
    (got,) = run(prog, tmp_path, [("backoff", "FPPF" + "RF" + "RP")])
    assert got == model_backoff("FPPF" + "RF" + "RP") == ["1:2:1", "0:1:1", "0:0:1", "1:4:2", "1:2:1", "1:0:0"]
    # disabled: not taken, nothing counted down; enabled again, the back-off goes on where it was
    (got,) = run(prog, tmp_path, [("backoff", "FDPPPEPPP")])
    assert got == model_backoff("FDPPPEPPP") == ["1:2:1", "0:2:1", "0:2:1", "0:2:1", "0:1:1", "0:0:1", "1:0:0"]


def test_seeded_random_sweep(prog, tmp_path):
    rnd = random.Random(20261021)
    cmds, want = [], []
    for _ in range(2000):
        r = rnd.choice((64, 256, 4096, R))
        tri_max, wide_max = rnd.choice((0, r // 8, r // 4)), rnd.choice((0, r // 32, r // 4))
        u = rnd.randint(1, 40)
        n = rnd.choice((2 * u, rnd.randint(2 * u, 40 * r), rnd.randint(2 * u, 3 * r)))
        group, auto, tri = rnd.choice((2, 3, 16, 16, 16, 64)), rnd.random() < 0.8, rnd.random() < 0.8
        G = chunk_size(n, u, group, auto, r, tri, tri_max, wide_max)
        assert group <= G <= (4 * group if auto else group)             # each rule at most doubles
        cmds.append(size_cmd(n, u, group, auto, r, tri, tri_max, wide_max)); want.append([str(G), str(bound(n, G, u))])
    for _ in range(50):
        ops = "".join(rnd.choice("PPFFFRED"[:rnd.choice((3, 5, 8))]) for _ in range(rnd.randint(1, 120)))
        cmds.append(("backoff", ops)); want.append(model_backoff(ops))
    assert run(prog, tmp_path, cmds) == want
