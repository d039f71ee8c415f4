"""What the tests of the aggregate verify over ragged groups by random linear combination share: the Python models of the weight
derivation and of the plan (bls-bn254_amd/csrc/aggregate_rlc.h, aggregate_rlc_plan.h), the names the feature adds, and the
groups of signed pairs the GPU tests run it on."""
import hashlib

from tests import synth

AGR_KERNELS = ("k_agr_group", "k_agr_weigh", "k_agr_items", "k_agr_bits")
AGR_SYMBOLS = ("blsbn254_aggregate_verify_batch_rlc", "blsbn254_set_aggregate_rlc_segments", "blsbn254_aggregate_rlc_stats")
AGR_STATS = ("calls", "round1_groups", "round2_groups", "exact_groups", "ineligible_groups", "equations", "exact_calls", "failed_segments")
S_MAX = 16                                                              # aggregate_rlc_plan.h AGR_SMAX
MAX_KEYS = 1 << 16                                                      # host_common.h PREP_MAX_KEYS


def weight_of_digest(dg):
    a, b = int.from_bytes(dg[:4], "big"), int.from_bytes(dg[4:8], "big")
    return (a, b) if (a or b) else (1, 0)


def weight(seed, g, sig):
    """(a_g, b_g): r_g = a_g + b_g lambda"""
    return weight_of_digest(hashlib.sha256(seed + b"AGRLC" + g.to_bytes(8, "little") + sig).digest())


def pair_groups(off):
    return [g for g in range(len(off) - 1) for _ in range(off[g + 1] - off[g])]


def keys_repeat(N, u, max_keys=MAX_KEYS):
    return u * 2 <= N and u + 1 <= max_keys


def segments(setting, N, u, G, s_max=S_MAX):
    """S of the second round; 1: the round is skipped"""
    S = setting if setting else min(s_max, N // (2 * u) if u else 0)
    S = min(S, G)
    return 1 if S < 2 else S


def cut(G, S):
    """(bounds, segment of every group): consecutive groups, sizes that differ by at most one"""
    bound = [s * G // S for s in range(S + 1)]
    return bound, [s for s in range(S) for _ in range(bound[s], bound[s + 1])]


MERGE_GAP = 1 << 16                                                     # aggregate_rlc_plan.h AGR_MERGE_GAP


def failed_ranges(bound, passed, elig, off=None, merge_gap=0):
    """(eligible groups inside, [first, second) ranges): failed segments, adjacent ones merged, trimmed to eligible groups; two
    ranges with fewer than merge_gap pairs and signatures between them (off: the group offsets) become one"""
    out, s, S = [], 0, len(bound) - 1
    while s < S:
        if passed[s]:
            s += 1
            continue
        e = s
        while e < S and not passed[e]:
            e += 1
        a, b = bound[s], bound[e]
        while a < b and not elig[a]:
            a += 1
        while b > a and not elig[b - 1]:
            b -= 1
        if a < b:
            if out and off[a] - off[out[-1][1]] + a - out[-1][1] < merge_gap:
                out[-1] = (out[-1][0], b)
            else:
                out.append((a, b))
        s = e
    return sum(1 for a, b in out for g in range(a, b) if elig[g]), out


SEED = bytes(range(1, 33))


class Data:
    """sizes[g] pairs per group: pair i of the call uses key i mod pool and a message of its own; every group's aggregate is the
    engine's sum of its pairs' signatures (an empty group: the first pair's signature, a valid point)"""
    def __init__(self, e, sizes, dst, pool=8, salt=0):
        n = sum(sizes)
        skb = [synth.sk_of(k).to_bytes(32, "big") for k in range(pool)]
        pk_pool = e.sk_to_pk_batch(b"".join(skb), pool)
        msgs = [synth.msg_of((salt << 20) + i) for i in range(n)]
        sigs = e.sign_batch(b"".join(skb[i % pool] for i in range(n)), msgs, dst)
        self.dst, self.sizes = dst, list(sizes)
        self.keys, self.msgs, self.sigs = [], [], []
        pos = 0
        for k in sizes:
            self.keys.append([pk_pool[128 * (i % pool):128 * (i % pool) + 128] for i in range(pos, pos + k)])
            self.msgs.append(msgs[pos:pos + k])
            self.sigs.append(e.aggregate_sigs(sigs[64 * pos:64 * (pos + k)], k) if k else sigs[:64])
            pos += k

    def flip_message(self, g, j=0):
        m = self.msgs[g][j]
        self.msgs[g][j] = bytes([m[0] ^ 1]) + m[1:]

    def args(self):
        return [b"".join(k) for k in self.keys], self.msgs, b"".join(self.sigs), self.dst
