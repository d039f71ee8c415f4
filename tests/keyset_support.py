"""What the tests of the key-set call families share: the registries with special keys (Committee, World), the contributions of
the merge calls (Con), signing helpers, the wire-format helpers, and the Python models of the host-side plans that both the
host-side and the GPU tests compare against."""
import random

from tests import synth
from tests.helpers import IDENT1, IDENT2, b32, row_of

R = synth.R
ST_SHORT = 5
STATS = ("optimistic_groups", "fallback_groups", "verified_contributions", "short_groups")


class Committee:
    """n keys [sk_i] G2gen made on the GPU.  special (n >= 33): an identity key, an off-curve key, an undecodable key, P and -P,
    one key at two indices and a key outside the r-torsion.  sk[i]: what key i adds to a group's secret key (None: no
    signature can verify with it selected)."""

    def __init__(self, eng, n, seed, special=True):
        self.n = n
        self.sk = [synth.sk_of(1000 * seed + k) for k in range(n)]
        pk = eng.sk_to_pk_batch(b"".join(map(b32, self.sk)), n)
        self.keys = [pk[128 * i:128 * i + 128] for i in range(n)]
        self.bad, self.at = set(), {}
        if special and n >= 33:
            at = self.at = {"ident": 3, "off": 5, "undec": n - 2, "p": 7, "negp": n // 2, "dup_a": 1, "dup_b": n - 1, "nonsub": 9}
            self.keys[at["ident"]] = IDENT2; self.sk[at["ident"]] = 0
            off = bytearray(self.keys[at["off"]]); off[127] ^= 1
            self.keys[at["off"]] = bytes(off)
            self.keys[at["undec"]] = b"\xff" * 32 + self.keys[at["undec"]][32:]
            self.bad = {at["off"], at["undec"]}
            p = self.keys[at["p"]]
            self.keys[at["negp"]] = p[:64] + b32(synth.P - int.from_bytes(p[64:96], "big")) + b32(synth.P - int.from_bytes(p[96:], "big"))
            self.sk[at["negp"]] = R - self.sk[at["p"]]
            self.keys[at["dup_b"]] = self.keys[at["dup_a"]]; self.sk[at["dup_b"]] = self.sk[at["dup_a"]]
            self.keys[at["nonsub"]] = synth.NON_SUBGROUP_PK
            for i in self.bad | {at["nonsub"]}:
                self.sk[i] = None
        self.pks = b"".join(self.keys)
        self.unsignable = {i for i in range(n) if self.sk[i] is None}

    def gather(self, sel):
        return b"".join(self.keys[i] for i in sorted(sel))

    def group_sk(self, sel):
        s = sum(self.sk[i] for i in sel if self.sk[i] is not None) % R
        return s or 1                                                  # (no signature verifies under the identity key anyway)


def sign_rows(eng, com, rows, msgs, dst):
    return bytearray(eng.sign_batch(b"".join(b32(com.group_sk(r)) for r in rows), msgs, dst))


def edge_rows(com, rnd):
    """about 24 rows (sets of indices) and the names of the ones later tests refer to"""
    n, named = com.n, {}
    good = [i for i in range(n) if i not in com.unsignable]
    rows = [set(), set(range(n)), {n - 1}]
    for w in range(min((n + 31) // 32, 3)):
        rows.append({32 * w}); rows.append({min(32 * w + 31, n - 1)})
    rows.append(set(rnd.sample(range(n), n // 2)))                      # exactly n/2 bits: not flipped
    named["boundary"] = len(rows); rows.append(set(rnd.sample(good, min(len(good), n // 2 + 1))))      # n/2 + 1 bits: the flip boundary, verifies
    rows.append(set(good))                                              # flipped, the bad keys left unselected: stays valid
    for dens in (0.1, 0.5, 0.9):
        rows.append({i for i in good if rnd.random() < dens})
        rows.append({i for i in range(n) if rnd.random() < dens})
    if com.at:
        at = com.at
        named["flipped_with_bad"] = len(rows); rows.append(set(range(n)) - {at["undec"], at["nonsub"]})     # flipped and selects the off-curve key
        named["p_negp"] = len(rows); rows.append({at["p"], at["negp"]})
        named["nonsub"] = len(rows); rows.append({0, at["nonsub"]})
        named["dup"] = len(rows); rows.append({at["dup_a"], at["dup_b"]})
        named["ident"] = len(rows); rows.append({0, 2, at["ident"]})
        rows.append({at["undec"]}); rows.append({0, at["off"]})
    named["tampered"] = len(rows); rows.append(set(good[:max(1, len(good) // 3)]))
    named["ident_sig"] = len(rows); rows.append(set(good[:max(1, len(good) // 4)]))
    return rows, named


def sign_sets(eng, com, sets, msgs, dst, sk=None):
    """one dict {key index: signature of that key on msgs[g]} per set of indices; sk(g, i) overrides the signing key"""
    pairs = [(g, i) for g, s in enumerate(sets) for i in sorted(s)]
    out = [dict() for _ in sets]
    if pairs:
        sks = b"".join(b32((sk(g, i) if sk else None) or com.sk[i] or 1) for g, i in pairs)
        sig = bytes(eng.sign_batch(sks, [msgs[g] for g, _ in pairs], dst))
        for k, (g, i) in enumerate(pairs):
            out[g][i] = sig[64 * k:64 * k + 64]
    return out


def good_keys(com):
    return [i for i in range(com.n) if i not in com.unsignable and i != com.at.get("ident")]


def delta(st1, st0):
    return {k: st1[k] - st0[k] for k in st1}


class World:
    """140 keys with an identity key (3), an off-curve key (5), a key outside the r-torsion (9), an undecodable key (138), P and
    -P (7, 70), one key at two indices (1, 139) and, on the checked handle, a key whose proof fails (12).  Committees of 1, 31,
    32, 33, 65 and 129 members: 1 and 2 overlap, 3 lists its members in descending order, 4 contains every special key."""

    def __init__(self, eng, M):
        self.dst = M.DEFAULT_DST
        self.n = n = 140
        rnd = random.Random(2027)
        self.reg = reg = Committee(eng, n, 64)
        at = reg.at
        first = [reg.sk[i] if reg.sk[i] else 1000 + i for i in range(n)]
        p = eng.pop_prove_batch(b"".join(b32(s) for s in first), n)
        self.proofs = p[:64 * 12] + IDENT1 + p[64 * 13:]
        self.special = set(at.values()) | {12}
        plain = [i for i in range(n) if i not in self.special]
        bad_com = sorted(self.special) + plain[20:20 + 65 - len(self.special)]
        rnd.shuffle(bad_com)
        self.coms = [[20], list(range(30, 61)), list(range(50, 82)), list(range(132, 99, -1)), bad_com, rnd.sample(plain, 129)]
        assert [len(c) for c in self.coms] == [1, 31, 32, 33, 65, 129]
        assert set(self.coms[1]) & set(self.coms[2]) and self.special <= set(self.coms[4]) and len(self.special) == 9
        # members whose entry is a candidate on both handles when its signature is honest
        self.clean = [[j for j, i in enumerate(mem) if i not in self.special or i in (at["p"], at["dup_a"], at["dup_b"])] for mem in self.coms]

    def keyset(self, M, e, checked, table=None):
        ks = M.KeySet(e, self.reg.pks, self.n, proofs=self.proofs if checked else None)
        ks.set_committees(self.coms if table is None else table)
        return ks

    def pos_of(self, c, key):
        return self.coms[c].index(key)


def sign_positions(eng, W, com, pos_sets, msgs, sk=None, coms=None):
    """one dict {position: signature of that member on msgs[g]} per group; sk(g, position) overrides the signing key"""
    coms = coms or W.coms
    sets = [{coms[c][p] for p in ps} for c, ps in zip(com, pos_sets)]
    by_key = sign_sets(eng, W.reg, sets, msgs, W.dst, sk=(lambda g, i: sk(g, coms[com[g]].index(i))) if sk else None)
    return [{p: by_key[g][coms[c][p]] for p in ps} for g, (c, ps) in enumerate(zip(com, pos_sets))]


def compact(mem, wide_row):
    r = bytearray((len(mem) + 7) // 8)
    for j, i in enumerate(mem):
        if (wide_row[i >> 3] >> (i & 7)) & 1:
            r[j >> 3] |= 1 << (j & 7)
    return bytes(r)


class Con:
    """one contribution: the keys its row names, the keys whose secrets sign it (signed, default the same; sk_delta is added to
    their sum), and what the test made of it: cand = the call may select it, good = it verifies on its own"""

    def __init__(self, keys, signed=None, sk_delta=0, cand=True, good=True):
        self.keys, self.signed, self.sk_delta, self.cand, self.good, self.sig = set(keys), signed, sk_delta, cand, good, None

    def broken(self, sig):
        self.sig, self.cand, self.good = sig, False, False
        return self


def sign_all(eng, com, groups, msgs, dst):
    flat = [(g, c) for g, cs in enumerate(groups) for c in cs]
    if flat:
        sks = b"".join(b32((com.group_sk(c.keys if c.signed is None else c.signed) + c.sk_delta) % R or 1) for _, c in flat)
        sig = bytes(eng.sign_batch(sks, [msgs[g] for g, _ in flat], dst))
        for k, (_, c) in enumerate(flat):
            c.sig = sig[64 * k:64 * k + 64]
    return groups


def as_args(groups, n=None):
    """what the wrapper takes: key indices, or row bytes where n is given"""
    return [[(row_of(c.keys, n) if n else sorted(c.keys), c.sig) for c in cs] for cs in groups]


def greedy(cs, admit):
    union, used = set(), []
    for c in cs:
        u = bool(admit(c)) and not (c.keys & union)
        if u:
            union |= c.keys
        used.append(u)
    return used, union


def expect(cs, kind=None):
    """the model: (used flags, union or None for a short group, went to the fallback, contributions verified there).
    kind: "cancel" = the selected errors cancel in the sum, "zero_sum" = the kept keys sum to the identity"""
    used, union = greedy(cs, lambda c: c.cand)
    if not any(used):
        return [False] * len(cs), None, False, 0
    if kind != "zero_sum" and (kind == "cancel" or all(c.good for c, u in zip(cs, used) if u)):
        return used, union, False, 0
    verified = sum(1 for c in cs if c.cand)
    used, union = greedy(cs, lambda c: c.cand and c.good)
    if not any(used) or kind == "zero_sum":
        return [False] * len(cs), None, True, verified
    return used, union, True, verified


def chunks(keys, sizes):
    out, at = [], 0
    for s in sizes:
        out.append(keys[at:at + s]); at += s
    assert all(len(c) == s for c, s in zip(out, sizes))
    return out


def com_args(coms, com, groups, as_rows=False):
    """what the wrapper takes: a contribution's keys as positions in its group's committee, or as a committee-wide row"""
    out = []
    for c, cs in zip(com, groups):
        at = {k: j for j, k in enumerate(coms[c])}
        pos = [sorted(at[k] for k in x.keys) for x in cs]
        out.append([(row_of(p, len(coms[c])) if as_rows else p, x.sig) for p, x in zip(pos, cs)])
    return out


def keys_of(W, c, positions=None):
    return [W.coms[c][j] for j in (W.clean[c] if positions is None else positions)]


def compress_entries(e, entries):
    """[{slot: 64 bytes}] -> [{slot: 32 bytes}]"""
    flat = [(g, k) for g, es in enumerate(entries) for k in sorted(es)]
    c = e.g1_compress_batch(b"".join(entries[g][k] for g, k in flat), len(flat)) if flat else b""
    out = [dict() for _ in entries]
    for j, (g, k) in enumerate(flat):
        out[g][k] = c[32 * j:32 * j + 32]
    return out


def compressed(e, sigs64):
    return e.g1_compress_batch(sigs64, len(sigs64) // 64) if sigs64 else b""


ITEM_GROUPS, PART_MAX = 64, 1 << 20         # keyset_committee_plan.h


def words(size):
    return (size + 31) // 32


def committee_model_plan(coms, com, chunk):
    """the plan of keyset_committee_plan.h in Python: (order, launches as (lo, hi, partials), items as (cword, mbase, first, count))"""
    sizes = [len(c) for c in coms]
    off, wbase = [0], [0]
    for s in sizes:
        off.append(off[-1] + s); wbase.append(wbase[-1] + words(s))
    order = sorted(range(len(com)), key=lambda g: com[g])               # Python's sort is stable
    part_max = min(PART_MAX, chunk)
    launches, items, lo = [], [], 0
    while lo < len(order):
        hi, part = lo, 0
        while hi < len(order) and hi - lo < chunk:
            w = words(sizes[com[order[hi]]])
            if hi > lo and part + w > part_max:
                break
            part += w; hi += 1
        a = lo
        while a < hi:
            c = com[order[a]]
            b = a
            while b < hi and com[order[b]] == c:
                b += 1
            for f in range(a, b, ITEM_GROUPS):
                for w in range(words(sizes[c])):
                    items.append((wbase[c] + w, off[c] + 32 * w, f, min(ITEM_GROUPS, b - f)))
            a = b
        launches.append((lo, hi, part))
        lo = hi
    return order, launches, items


def rlc_model_plan(msgs, C):
    """the plan of keyset_rlc_plan.h in Python: (order, chunks as (start, len, class), representatives)"""
    ids, rep = {}, []
    cls = []
    for g, m in enumerate(msgs):
        m = bytes(m)
        if m not in ids:
            ids[m] = len(ids); rep.append(g)
        cls.append(ids[m])
    order = sorted(range(len(msgs)), key=lambda g: cls[g])              # Python's sort is stable
    chunks, at = [], 0
    for k in range(len(rep)):
        size = cls.count(k)
        chunks += [(at + s, min(C, size - s), k) for s in range(0, size, C)]
        at += size
    return order, chunks, rep
