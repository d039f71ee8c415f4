"""CPU-only: the lane functions of the stake weights over a registered key set (bls-bn254_amd/csrc/keyset_weight.h) and the
plain C++ of their host side (keyset_weight_plan.h) compiled for the host into a stand-alone program
(tests/hostsim/keyset_weight_host.cpp), a wave run as 64 lane states with the halves of the reduction carried by the harness:
the key-major table, the sums over random rows at every row width at which the code takes another path against
Python integers, the column-total check at its boundary, the launch plan, and the repack of the groups that reach quorum.
A test tool; the product has no CPU path."""
import os
import random
import subprocess

import pytest

from tests import hostsim_build
from tests.helpers import row_of

M64 = (1 << 64) - 1
# n_keys -> (words, row bytes): one key; one word and a bit; three words and 9-byte rows; 64 words, every lane one word; 66
# words, lanes 0 and 1 own two (261-byte rows); 130 words, lanes 0 and 1 own three
WIDTHS = {1: (1, 1), 33: (2, 5), 70: (3, 9), 2035: (64, 255), 2081: (66, 261), 4133: (130, 517)}


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = hostsim_build.build("keyset_weight_host.cpp", "keyset_weight_host", shared=False)
    d = tmp_path_factory.mktemp("kw")

    def f(commands):
        """commands: lists of tokens -> per command the result line's tokens (without the command's name)"""
        path = os.path.join(str(d), "commands.txt")
        with open(path, "w") as fh:
            fh.write("\n".join(" ".join(str(t) for t in c) for c in commands) + "\n")
        out = subprocess.run([exe, path], check=True, stdout=subprocess.PIPE).stdout.decode().splitlines()
        assert len(out) == len(commands) and all(o.split()[0] == c[0] for o, c in zip(out, commands))
        return [o.split()[1:] for o in out]
    return f


def hexs(b):
    return bytes(b).hex() or "-"


def unhex(t):
    return b"" if t == "-" else bytes.fromhex(t)


def table(rnd, n, nc):
    """columns whose sums fit 64 bits, with entries that carry across the 32-bit halves"""
    pool = [0, 1, (1 << 32) - 1, 1 << 32, M64 // n]
    return [[rnd.choice(pool) for _ in range(n)] for _ in range(nc)]


@pytest.mark.parametrize("n", sorted(WIDTHS))
def test_widths(n):
    assert ((n + 31) // 32, (n + 7) // 8) == WIDTHS[n]


@pytest.mark.parametrize("n", sorted(WIDTHS))
def test_sums_against_python_integers(run, n):
    rnd = random.Random(4100 + n)
    W = (n + 31) // 32
    edge = sorted({k for w in (0, 1, 63, 64, 65, 127, 128, W - 1) if w < W for k in (32 * w, min(32 * w + 31, n - 1))})
    invalid = {edge[-1], edge[len(edge) // 2]} if n > 1 else set()
    valid = bytes(0 if i in invalid else 1 for i in range(n))
    rows = [set(), set(range(n)), {n - 1}, {0}, set(edge), set(invalid), set(range(n)) - invalid]
    rows += [{i for i in range(n) if rnd.random() < d} for d in (0.02, 0.3, 2 / 3, 0.97)]
    G = len(rows)
    rowhex = hexs(b"".join(row_of(r, n) for r in rows))
    cmds, want = [], []
    for nc in (1, 3, 8):
        cols = table(rnd, n, nc)
        flat = [v for col in cols for v in col]
        exp = [[sum(cols[q][i] for i in r if valid[i]) for q in range(nc)] for r in rows]
        assert all(v <= M64 for e in exp for v in e) and (n == 1 or any(v >> 32 for e in exp for v in e))
        for cuts in ([], [1, 4], list(range(1, G))):
            edges = [0] + cuts + [G]
            for lo, hi in zip(edges, edges[1:]):
                cmds.append(["weight", n, nc, G, lo, hi - lo, hexs(valid)] + flat + [rowhex])
                want.append([str(v) for e in exp[lo:hi] for v in e])
        cmds.append(["major", n, nc] + flat)
        want.append([str(cols[q][i]) for i in range(n) for q in range(nc)])
        if invalid:                                                     # plain arithmetic would lend an invalid key's stake
            assert exp[5] == [0] * nc and exp[1] == exp[6]
    assert run(cmds) == want


def test_carries_cross_the_halves_in_every_round(run):
    """64 words, one key per lane, every key 2^32 - 1 and then 2^32 + 1: each round of the reduction carries from the low half
    into the high half in some lane; and a single 2^64 - 1 arrives from the last lane untouched"""
    n = 2048
    rows = hexs(row_of(range(0, n, 32), n) + row_of([n - 1], n))
    valid = hexs(bytes([1]) * n)
    cmds, want = [], []
    for v in ((1 << 32) - 1, (1 << 32) + 1):
        cmds.append(["weight", n, 1, 2, 0, 2, valid] + [v] * n + [rows]); want.append([str(64 * v), str(v)])
    cmds.append(["weight", n, 2, 2, 0, 2, valid] + [0] * (n - 1) + [M64] + [0] * (n - 32) + [1 << 63] + [0] * 31 + [rows])
    want.append(["0", str(1 << 63), str(M64), "0"])
    assert run(cmds) == want


def test_column_totals_at_the_boundary(run):
    n = 5
    ok = [M64 - 10, 3, 0, 7, 0]                                         # 2^64 - 1
    over = [M64 - 10, 3, 1, 7, 0]                                       # 2^64
    small = [1, 2, 3, 4, 5]
    res = run([["fit", n, 1] + ok, ["fit", n, 1] + over, ["fit", n, 3] + small + ok + small, ["fit", n, 3] + small + ok + over,
               ["fit", n, 2] + over + over, ["fit", 1, 1, M64], ["fit", 2, 1, M64, 1], ["fit", 2, 2, 1 << 63, 1 << 63, (1 << 63) - 1, 1 << 63]])
    assert sum(ok) == M64 and sum(over) == M64 + 1
    assert [int(r[0]) for r in res] == [-1, 0, -1, 2, 0, -1, 0, 0]


def test_launch_plan(run):
    res = run([["plan", 41, 1 << 22], ["plan", 41, 512], ["plan", 41, 64], ["plan", 41, 10], ["plan", 9, 256], ["plan", 8, 256], ["plan", 1, 64]])
    assert [[int(t) for t in r] for r in res] == [[65536, 1], [8, 6], [1, 41], [1, 41], [4, 3], [4, 2], [1, 1]]


@pytest.mark.parametrize("lead", [0, 7])
def test_repack_of_reaching_groups(run, lead):
    rnd = random.Random(31 + lead)
    n, G, nc = 70, 6, 2
    rb = (n + 7) // 8
    rows = [bytes(rnd.randrange(256) for _ in range(rb)) for _ in range(G)]
    sigs = [bytes(rnd.randrange(256) for _ in range(64)) for _ in range(G)]
    msgs = [b"first", b"", b"three", b"4", b"", b"the last one"]
    base = bytes(rnd.randrange(256) for _ in range(lead))               # the call's offsets start behind these bytes
    off = [lead]
    for m in msgs:
        off.append(off[-1] + len(m))
    minw = [10, 5]
    cases = {"all": [[10, 5]] * G, "none": [[9, 5], [10, 4], [0, 0], [9, 100], [100, 4], [0, 5]],
             "first and last": [[10, 5], [9, 9], [11, 4], [0, 0], [9, 5], [M64, M64]],
             "some": [[9, 5], [10, 5], [11, 6], [10, 4], [M64, 5], [0, M64]]}
    sub_bits = bytes([0b101101, 0])                                     # bits of the sub-call's groups 0, 2, 3, 5
    for name, w in cases.items():
        reach = [g for g in range(G) if all(w[g][q] >= minw[q] for q in range(nc))]
        cmd = ["quorum", G, nc, rb] + minw + [v for g in w for v in g] + off + [hexs(b"".join(rows)), hexs(b"".join(sigs)), hexs(base + b"".join(msgs)), hexs(sub_bits)]
        r = run([cmd])[0]
        cnt = int(r[0])
        assert cnt == len(reach) and [int(t) for t in r[1:1 + cnt]] == reach, name
        want_off = [0]
        for g in reach:
            want_off.append(want_off[-1] + len(msgs[g]))
        assert [int(t) for t in r[1 + cnt:2 + 2 * cnt]] == want_off, name
        got_rows, got_sigs, got_msgs, bm = map(unhex, r[2 + 2 * cnt:])
        assert got_rows == b"".join(rows[g] for g in reach) and got_sigs == b"".join(sigs[g] for g in reach), name
        assert got_msgs == b"".join(msgs[g] for g in reach), name
        want_bm = 0
        for j, g in enumerate(reach):
            if (sub_bits[0] >> j) & 1:
                want_bm |= 1 << g
        assert bm == bytes([want_bm]), name
    assert {len([g for g in range(G) if all(w[g][q] >= minw[q] for q in range(nc))]) for w in cases.values()} == {6, 0, 2, 3}
    # a minimum of 0 switches a column off
    r = run([["quorum", 2, 2, 1, 0, 3, 0, 3, 0, 2, 0, 0, 0, "0102", hexs(bytes(128)), "-", "03"]])[0]
    assert r[:2] == ["1", "0"]
