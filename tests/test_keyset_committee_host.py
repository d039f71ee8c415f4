"""CPU-only: the plan and the checks of the committees over a registered key set (bls-bn254_amd/csrc/keyset_committee_plan.h) and
their lane functions (keyset_committee.h) compiled for the host with -DBN_CHECK into a stand-alone program
(tests/hostsim/keyset_committee_host.cpp): the plan against a Python model and against its own invariants, the committee words,
the flip threshold at the committee's size, the whole sum pipeline (gather, word sums, the segmented levels, the complement,
the unsort) against the pure-Python curve arithmetic, and the refusals of a table.  A test tool; the product has no CPU path."""
import os
import random
import subprocess

import pytest

from tests import hostsim_build
from tests.helpers import IDENT2, row_of
from tests.keyset_support import ITEM_GROUPS, PART_MAX, committee_model_plan, words



@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = hostsim_build.build("keyset_committee_host.cpp", "keyset_committee_host", shared=False)
    d = tmp_path_factory.mktemp("kc")

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


def set_cmd(n_keys, coms):
    off = [0]
    for c in coms:
        off.append(off[-1] + len(c))
    return ["set", n_keys, len(coms)] + off + [i for c in coms for i in c]


def parse_plan(tok, G):
    v = [int(t) for t in tok]
    nl, ni = v[0], v[1]
    order, spbase, srow = v[2:2 + G], v[2 + G:2 + 2 * G], v[2 + 2 * G:2 + 3 * G]
    at = 2 + 3 * G
    launches = [tuple(v[at + 6 * i:at + 6 * i + 6]) for i in range(nl)]
    at += 6 * nl
    items = [tuple(v[at + 4 * i:at + 4 * i + 4]) for i in range(ni)]
    assert at + 4 * ni == len(v)
    return order, spbase, srow, launches, items


COMS = [[5], list(range(31)), list(range(10, 42)), list(range(69, 36, -1)), list(range(64)), list(range(5, 70)), [0, 69, 33]]
assert [len(c) for c in COMS] == [1, 31, 32, 33, 64, 65, 3]


@pytest.mark.parametrize("chunk", [1 << 22, 512, 64, 8, 2])
def test_plan_against_the_model_and_its_invariants(run, chunk):
    rnd = random.Random(chunk)
    com = [rnd.randrange(len(COMS)) for _ in range(150)] + [5] * 70 + [rnd.randrange(len(COMS)) for _ in range(30)]
    rnd.shuffle(com)
    G = len(com)
    res = run([set_cmd(70, COMS), ["plan", chunk, G] + com])
    assert res[0][:2] == ["ok", str(len(COMS))]
    order, spbase, srow, launches, items = parse_plan(res[1], G)
    sizes = [len(c) for c in COMS]
    m_order, m_launches, m_items = committee_model_plan(COMS, com, chunk)
    assert order == m_order and items == m_items
    assert [(lo, hi, p) for lo, hi, _, _, p, _ in launches] == m_launches
    # the permutation is stable
    assert sorted(order) == list(range(G))
    assert all((com[a], a) < (com[b], b) for a, b in zip(order, order[1:]))
    # the rows follow one another in the caller's order
    rb = [(sizes[c] + 7) // 8 for c in com]
    assert [srow[i] for i in range(G)] == [sum(rb[:order[i]]) for i in range(G)]
    # launches: sorted-group boundaries, both limits, the partials group-major and dense
    assert launches[0][0] == 0 and launches[-1][1] == G and all(a[1] == b[0] for a, b in zip(launches, launches[1:]))
    wbase = [sum(words(s) for s in sizes[:c]) for c in range(len(COMS))]
    for lo, hi, item0, n_items, part, levels in launches:
        assert 0 < hi - lo <= chunk
        assert part <= min(PART_MAX, chunk) or hi - lo == 1
        base = 0
        for i in range(lo, hi):
            assert spbase[i] == base
            base += words(sizes[com[order[i]]])
        assert base == part and levels >= 1
        # every (group, word) of the launch is covered by exactly one item; no item spans two committees or more than 64 groups
        seen = set()
        for cword, mbase, first, count in items[item0:item0 + n_items]:
            assert 1 <= count <= ITEM_GROUPS and lo <= first and first + count <= hi
            cs = {com[order[i]] for i in range(first, first + count)}
            assert len(cs) == 1
            c = cs.pop()
            w = cword - wbase[c]
            assert 0 <= w < words(sizes[c]) and mbase == sum(sizes[:c]) + 32 * w
            for i in range(first, first + count):
                assert (i, w) not in seen
                seen.add((i, w))
        assert seen == {(i, w) for i in range(lo, hi) for w in range(words(sizes[com[order[i]]]))}
    assert sum(l[3] for l in launches) == len(items)


def test_runs_of_65_and_129_groups(run):
    """one committee of 65 members (3 words): 64, 65, 128 and 129 groups give 1, 2, 2 and 3 items per word"""
    cmds = [set_cmd(70, COMS)]
    for G in (64, 65, 128, 129):
        cmds.append(["plan", 1 << 22, G] + [5] * G)
    res = run(cmds)
    for G, tok, per_word in zip((64, 65, 128, 129), res[1:], (1, 2, 2, 3)):
        _, _, _, launches, items = parse_plan(tok, G)
        assert len(launches) == 1 and len(items) == 3 * per_word
        for w in range(3):
            mine = [it for it in items if it[0] == 3 + 4 + w]           # word base of committee 5: 1 + 1 + 1 + 2 + 2
            assert len(mine) == per_word and sum(it[3] for it in mine) == G
            assert [it[2] for it in mine] == list(range(0, G, 64))


def test_committee_words(run):
    """a committee that lists its keys in descending order, and one that straddles a bad key: bit j of a committee word is
    the bit of key members[j]"""
    n = 70
    rnd = random.Random(3)
    bad = [1 if i in (5, 40, 68) else 0 for i in range(n)]
    skip = [1 if (bad[i] or i in (3, 41)) else 0 for i in range(n)]
    valid = [0 if (skip[i] or i == 9) else 1 for i in range(n)]
    coms = [list(range(69, 36, -1)), list(range(2, 9)), rnd.sample(range(n), 70), [40]]
    res = run([set_cmd(n, coms), ["words", n, hexs(bad), hexs(skip), hexs(valid)]])
    got = [int(t) for t in res[1]]
    W = sum(words(len(c)) for c in coms)
    assert len(got) == 3 * W
    for k, bits in enumerate((bad, skip, valid)):
        want = []
        for c in coms:
            for w in range(words(len(c))):
                want.append(sum(bits[i] << j for j, i in enumerate(c[32 * w:32 * w + 32])))
        assert got[k * W:(k + 1) * W] == want
    assert got[0] == 1 << (69 - 68) | 1 << (69 - 40) and got[2] == 1 << 3        # descending; {2..8} straddles key 5


@pytest.mark.parametrize("size", [1, 2, 31, 32, 33])
def test_flip_threshold_is_the_committees_size(run, size):
    half = size // 2
    cmds, want = [], []
    W = words(size)
    for pop in sorted({0, half, half + 1, size} & set(range(size + 1))):
        row = row_of(range(size - pop, size), size)                     # the LAST pop members
        for noflip in (0, 1):
            cmds.append(["count", size, noflip, hexs(row)] + [0] * W)
            want.append([str(int(2 * pop > size and not noflip)), "1"])
        # a bad member at the last position: ok only while it is not selected
        cbad = [0] * W
        cbad[(size - 1) // 32] = 1 << ((size - 1) % 32)
        cmds.append(["count", size, 0, hexs(row)] + cbad)
        want.append([str(int(2 * pop > size)), str(int(pop == 0))])
    assert run(cmds) == want


def key_set(B, n, rnd):
    pts = [B.g2_mul(B.G2_GEN, rnd.randrange(1, B.R)) for _ in range(10)]
    keys = [B.g2_to_bytes(pts[i] if i < 10 else B.g2_add(pts[i % 10], pts[(i // 10) % 10 - 1])) for i in range(n)]
    keys[3] = IDENT2
    off = bytearray(keys[5]); off[127] ^= 1
    keys[5] = bytes(off)
    keys[n - 2] = b"\xff" * 32 + keys[n - 2][32:]
    return keys, {5, n - 2}, {3}


@pytest.mark.parametrize("chunk", [1 << 22, 8])
def test_sums_against_the_curve_model(run, pyref, chunk):
    """70 keys with an identity, an off-curve and an undecodable key; committees that overlap, one in descending order, one
    across two words with the bad key: every row's sum equals the sum of the listed keys"""
    B = pyref
    n = 70
    rnd = random.Random(11)
    keys, bad, ident = key_set(B, n, rnd)
    skip = bad | ident
    coms = [[7], list(range(69, 36, -1)), list(range(0, 40)), [1, 2, 4, 6, 8, 3], list(range(30, 66))]
    sizes = [len(c) for c in coms]
    groups = []                                                          # (committee, set of member positions)
    for c, s in enumerate(sizes):
        full = set(range(s))
        badpos = {j for j, i in enumerate(coms[c]) if i in bad}
        groups += [(c, set()), (c, full), (c, set(rnd.sample(range(s), s // 2))), (c, full - badpos)]
        if s > 1:
            groups.append((c, set(rnd.sample(sorted(full - badpos), min(len(full - badpos), s // 2 + 1)))))
        if badpos:
            groups.append((c, {min(badpos)}))
    rnd.shuffle(groups)
    com = [c for c, _ in groups]
    rows = b"".join(row_of(r, sizes[c]) for c, r in groups)
    res = run([set_cmd(n, coms), ["sum", n, chunk, len(groups)] + com + [hexs(b"".join(keys)), hexs(rows)]])[1]
    pts = [None if i in skip else B.g2_from_bytes(keys[i])[1] for i in range(n)]
    flipped = 0
    for g, (c, r) in enumerate(groups):
        listed = [coms[c][j] for j in sorted(r)]
        want_ok = not (set(listed) & bad)
        want_flip = 2 * len(r) > sizes[c]
        flipped += want_flip
        acc = None
        if want_ok:
            for i in listed:
                if i not in skip:
                    acc = B.g2_add(acc, pts[i])
        assert res[3 * g:3 * g + 3] == [str(int(want_flip)), str(int(want_ok)), B.g2_to_bytes(acc).hex()], (g, c, sorted(r))
    assert flipped >= 5 and (int(res[-1]) > 3) == (chunk == 8)


def test_a_refused_table_leaves_the_old_one(run):
    n = 20
    good = [[0, 1, 2], [2, 3]]
    cmds = [set_cmd(n, good),
            set_cmd(n, [[0, 1], [4, 5, 4]]),                            # a duplicate inside a committee
            set_cmd(n, [[0, 1], [n]]),                                  # an index equal to n_keys
            ["set", n, 2, 0, 2, 2, 0, 1],                               # an empty committee
            ["set", n, 3, 0, 3, 2, 4, 0, 1, 2, 3],                      # decreasing offsets
            ["set", n, 1, 1, 2, 0, 1],                                  # offsets that do not start at 0
            ["plan", 64, 3, 1, 0, 1],
            set_cmd(n, [[0, 1], [1, 0], [0, 1, 2]])]                    # overlapping committees are fine
    res = run(cmds)
    assert res[0][:2] == ["ok", "2"]
    for r, what in zip(res[1:6], ("committee_1_lists_key_4_twice", "committee_1:_member_0_names_key_20", "committee_1_is_empty",
                                  "committee_1:_the_offsets_decrease", "committee_0:_the_offsets_do_not_start_at_0")):
        assert r[:2] == ["refused", "2"] and r[2].startswith(what), r
    order, _, _, _, items = parse_plan(res[6], 3)                       # still the first table: committee 1 has 2 members at offset 3
    assert order == [1, 0, 2] and items == [(0, 0, 0, 1), (1, 3, 1, 2)]
    assert res[7][:2] == ["ok", "3"]


def test_row_checks(run):
    coms = [list(range(13)), list(range(16))]
    r13, r16 = row_of([0, 12], 13), row_of([15], 16)
    pad = bytes([r13[0], r13[1] | 0x20])
    cmds = [set_cmd(20, coms),
            ["rows", 2, 0, 1, 0, 2, 4, hexs(r13 + r16)],
            ["rows", 2, 0, 2, 0, 2, 4, hexs(r13 + r16)],                # com[g] = n_com
            ["rows", 2, 0, 1, 0, 2, 3, hexs(r13 + r16)],                # a short row
            ["rows", 2, 1, 0, 0, 2, 4, hexs(r16 + pad)],                # a padding bit
            ["rows", 2, 0, 1, 0, 3, 5, hexs(r13 + b"\0" + r16)]]         # a long row
    assert [r[0] for r in run(cmds)[1:]] == ["-1", "1", "1", "1", "0"]
