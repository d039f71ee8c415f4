"""What the tests of the distinct-message rule (bls-bn254_amd/csrc/msg_distinct.h; blsbn254_hash_distinct_batch and the _distinct
forms of the aggregate verify over groups) share: the names the feature adds, the Python model of the rule and of its table, and
the groups of signed pairs the GPU tests run it on.  The reference of every expectation is existing code: the 64-byte outputs of
hash_to_g1_batch (or a CPU model of the map) compared with a Python set, and the parent's aggregate_verify_batch."""
from tests import synth

MD_KERNELS = ("k_md_keys", "k_md_insert")
MD_SYMBOLS = ("blsbn254_hash_distinct_batch", "blsbn254_aggregate_verify_batch_distinct", "blsbn254_aggregate_verify_batch_rlc_distinct",
              "blsbn254_msg_distinct_stats")
MD_STATS = ("calls", "pairs", "repeated_groups", "slots")
EMPTY = 0xffffffff                                                      # key_cache.h KC_EMPTY
AFFINE, HOMOGENEOUS = 0, 1                                              # msg_distinct.h MD_*
P = synth.P


def slots_for(n):
    """msg_distinct.h md_slots: the smallest power of two >= 2 n, at least 2"""
    m = 2
    while m < 2 * n:
        m <<= 1
    return m


def group_of(goff, i):
    """the group that owns pair i, None for a pair in front of the first group or behind the last"""
    for g in range(len(goff) - 1):
        if goff[g] <= i < goff[g + 1]:
            return g
    return None


def dup_of(points, goff):
    """THE rule: dup[g] = the points (any hashable: 64 bytes, (x, y)) of group g's pairs are not pairwise different"""
    return [len(set(points[goff[g]:goff[g + 1]])) != goff[g + 1] - goff[g] for g in range(len(goff) - 1)]


def table_model(points, goff, order, M, start):
    """(slots, dup) of md_insert's lanes run in `order` over a cleared table of M slots; start(g, i): the slot hash of pair i"""
    slots, dup = [EMPTY] * M, [0] * (len(goff) - 1)
    for i in order:
        g = group_of(goff, i)
        if g is None:
            continue
        s = start(g, i) & (M - 1)
        for _ in range(M):
            old = slots[s]
            if old == EMPTY:
                slots[s] = i
                break
            if group_of(goff, old) == g and points[old] == points[i]:
                dup[g] = 1
                break
            s = (s + 1) & (M - 1)
        else:
            dup[g] = 1                                                  # no free slot in M probes: fail closed
    return slots, dup


def and_not(valid, dup):
    return [v and not d for v, d in zip(valid, dup)]


class Signed:
    """Groups of honestly signed pairs with the messages the test names: msg_sets[g] = the messages of group g, pair i of the call
    signed by key i mod pool; every group's aggregate is the engine's sum of its pairs' signatures (an empty group: a valid
    point that signs nothing)."""
    def __init__(self, e, msg_sets, dst, pool=8):
        flat = [m for ms in msg_sets for m in ms]
        n = len(flat)
        skb = [synth.sk_of(k).to_bytes(32, "big") for k in range(pool)]
        pk_pool = e.sk_to_pk_batch(b"".join(skb), pool)
        sigs = e.sign_batch(b"".join(skb[i % pool] for i in range(n)), flat, dst) if n else b""
        spare = e.sign_batch(skb[0], [b"spare"], dst)
        self.dst, self.msgs = dst, [list(ms) for ms in msg_sets]
        self.keys, self.sigs = [], []
        pos = 0
        for ms in msg_sets:
            k = len(ms)
            self.keys.append(b"".join(pk_pool[128 * (i % pool):128 * (i % pool) + 128] for i in range(pos, pos + k)))
            self.sigs.append(e.aggregate_sigs(sigs[64 * pos:64 * (pos + k)], k) if k else spare)
            pos += k

    def goff(self):
        off = [0]
        for ms in self.msgs:
            off.append(off[-1] + len(ms))
        return off

    def flat(self):
        return [m for ms in self.msgs for m in ms]

    def args(self):
        return self.keys, self.msgs, b"".join(self.sigs), self.dst

    def corrupt(self, g):
        """group g's aggregate replaced by its neighbour's, another valid point: the group fails its equation"""
        self.sigs[g] = self.sigs[(g + 1) % len(self.sigs)]
