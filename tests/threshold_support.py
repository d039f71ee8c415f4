"""What the tests of the checked threshold combine share with the tests that run it beside other call families: a dealt set of
groups with every share's partial signature (Deal) and the ways to spoil one."""
import random

from tests import synth
from tests.helpers import IDENT1, b32, bits_of, poly_eval

R = synth.R
OTHER_MSG, NEIGHBOUR_KEY, IDENTITY, OFF_CURVE, UNDECODABLE = range(5)


def pack(sets):
    return [b"".join(map(b32, s)) for s in sets]


class Deal:
    """groups of sizes ns with thresholds ts: coefficients, ids (random in [1, r) in the even groups, 1 .. n in the odd ones
    unless small_ids), commitments, one message per group, and every share's partial signature, all of them good"""

    def __init__(self, eng, ns, ts, seed, dst, small_ids=False):
        rnd = random.Random(seed)
        self.ns, self.ts, self.dst, self.ng = list(ns), list(ts), dst, len(ns)
        self.coefs = [[rnd.randrange(1, R) for _ in range(t)] for t in ts]
        self.ids = [list(range(1, n + 1)) if (g & 1 or small_ids) else [rnd.randrange(1, R) for _ in range(n)] for g, n in enumerate(ns)]
        flat = [c for s in self.coefs for c in s]
        pks = eng.sk_to_pk_batch(b"".join(map(b32, flat)), len(flat))
        self.commits, pos = [], 0
        for t in ts:
            self.commits.append(pks[128 * pos:128 * (pos + t)]); pos += t
        self.msgs = [b"checked combine %d/%d" % (seed, g) for g in range(self.ng)]
        self.start = [0]
        for n in ns:
            self.start.append(self.start[-1] + n)
        self.N = self.start[-1]
        self.shares = [poly_eval(self.coefs[g], x) for g in range(self.ng) for x in self.ids[g]]
        self.sigs = bytearray(self.sign(eng, self.shares, [self.msgs[g] for g in range(self.ng) for _ in range(ns[g])]))

    def sign(self, eng, sks, msgs):
        return eng.sign_batch(b"".join(map(b32, sks)), msgs, self.dst) if sks else b""

    def spoil(self, eng, g, i, kind):
        """share i of group g becomes a bad partial of the given kind"""
        p = self.start[g] + i
        if kind == OTHER_MSG:
            s = self.sign(eng, [self.shares[p]], [self.msgs[g] + b" (another message)"])
        elif kind == NEIGHBOUR_KEY:
            j = p + 1 if i + 1 < self.ns[g] else p - 1
            s = self.sign(eng, [self.shares[j]], [self.msgs[g]])
        elif kind == IDENTITY:
            s = IDENT1
        elif kind == OFF_CURVE:
            s = bytearray(self.sigs[64 * p:64 * p + 64]); s[63] ^= 1
        else:
            s = b"\xff" * 32 + bytes(self.sigs[64 * p + 32:64 * p + 64])
        self.sigs[64 * p:64 * p + 64] = s

    def sig_sets(self, groups=None):
        return [bytes(self.sigs[64 * self.start[g]:64 * self.start[g + 1]]) for g in (range(self.ng) if groups is None else groups)]

    def args(self, groups=None):
        gs = list(range(self.ng)) if groups is None else list(groups)
        return ([self.commits[g] for g in gs], pack([self.ids[g] for g in gs]), self.sig_sets(gs), [self.msgs[g] for g in gs], self.dst)

    def group_bits(self, bitmap, g):
        return bits_of(bitmap, self.N)[self.start[g]:self.start[g + 1]]


# ---------------------------------------------------------------- 6. several launches
def checked_flow(eng, n_groups, bad_every, seed, dst):
    """n_groups x (n = 5, t = 3, ids 1 .. 5); every bad_every-th group holds one partial over another message among its first 3"""
    d = Deal(eng, [5] * n_groups, [3] * n_groups, seed, dst, small_ids=True)
    wrong = d.sign(eng, [d.shares[5 * g + (g // bad_every) % 3] for g in range(0, n_groups, bad_every)],
                   [d.msgs[g] + b" (another message)" for g in range(0, n_groups, bad_every)])
    for k, g in enumerate(range(0, n_groups, bad_every)):
        p = 5 * g + (g // bad_every) % 3
        d.sigs[64 * p:64 * p + 64] = wrong[64 * k:64 * k + 64]
    return d
