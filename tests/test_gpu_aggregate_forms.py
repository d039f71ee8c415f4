"""GPU tests (MI355X) that pin WHICH kernels the aggregate family runs off the raw per-key line tables: aggregate_verify (per-key
sums, or pair by pair where the keys do not repeat), aggregate_partial[_with_sig], aggregate_verify_prepared and both rounds of
aggregate_verify_batch_rlc.  Every case asserts the result (the oracle's boolean or Miller product), that exactly the named Miller
kernel ran, once, and no other, and the launches of fp12_mul_pairs -- the product tree's levels, ceil(log2(values)), which tells
one value per pair from one per two -- and of g2_prepare.  The sizes are the smallest that reach each branch of
launch_miller_raw (host_aggregate.hip), the one place the form is chosen."""
import pytest

from tests import synth
from tests.aggregate_rlc_support import Data, SEED
from tests.gpu_support import ENGINES, MILLER_KERNELS, PREP_KERNELS, eng, engines, launches, M  # noqa: F401 (fixtures)
from tests.helpers import bits_of, IDENT1

pytestmark = pytest.mark.gpu
RECORDED = MILLER_KERNELS + PREP_KERNELS + ("fp12_mul_pairs",)


def levels(values):
    """launches of fp12_mul_pairs by fp12_tree over that many Fp12 values"""
    return (values - 1).bit_length()


def record(miller, values, prepare, **more):
    """the launch record of a call: that Miller kernel once, the product tree over `values`, g2_prepare `prepare` times"""
    rec = {miller: 1, "fp12_mul_pairs": levels(values), "g2_prepare": prepare}
    rec.update(more)
    return {k: v for k, v in rec.items() if v}


def neg_g2(pk):
    """(x, -y) of an uncompressed G2 point"""
    y1, y0 = int.from_bytes(pk[64:96], "big"), int.from_bytes(pk[96:128], "big")
    return pk[:64] + ((synth.P - y1) % synth.P).to_bytes(32, "big") + ((synth.P - y0) % synth.P).to_bytes(32, "big")


class Pairs:
    """n pairs, pair i under key i mod pool of the seeded key sequence with a message of its own, and their aggregate signature"""
    def __init__(self, e, n, pool, dst, salt):
        skb = [synth.sk_of(k).to_bytes(32, "big") for k in range(pool)]
        pk = e.sk_to_pk_batch(b"".join(skb), pool)
        self.n, self.pool, self.dst = n, pool, dst
        self.key_pool = [pk[128 * k:128 * k + 128] for k in range(pool)]
        self.idx = [i % pool for i in range(n)]
        self.msgs = [synth.msg_of((salt << 20) + i) for i in range(n)]
        self.pks = b"".join(self.key_pool[k] for k in self.idx)
        self.agg = e.aggregate_sigs(e.sign_batch(b"".join(skb[k] for k in self.idx), self.msgs, dst), n)

    def damaged(self):
        """(label, pks, msgs, signature, distinct keys): the valid input, one damaged message, an identity signature, a key outside
        the subgroup in place of the last pair's"""
        bad = list(self.msgs); bad[self.n // 2] = b"tampered"
        out = self.pks[:128 * (self.n - 1)] + synth.NON_SUBGROUP_PK
        return [("valid", self.pks, self.msgs, self.agg, self.pool), ("message", self.pks, bad, self.agg, self.pool),
                ("identity_sig", self.pks, self.msgs, IDENT1, self.pool), ("outside_key", out, self.msgs, self.agg, len(set(self.idx[:-1])) + 1)]


@pytest.fixture(scope="module")
def few(eng, M):
    return Pairs(eng, 8, 3, M.DEFAULT_DST, 41)


@pytest.fixture(scope="module")
def repeated(eng, M):
    return Pairs(eng, 1024, 4, M.DEFAULT_DST, 42)


@pytest.fixture(scope="module")
def distinct(eng, M):
    return Pairs(eng, 1024, 1024, M.DEFAULT_DST, 43)


@pytest.fixture(scope="module")
def products(eng, oracle):
    """(the oracle's multi_miller_loop over the pairs of D, the same with the signature's pair (agg, -G2gen) behind them), once per D"""
    made = {}

    def get(D):
        if id(D) not in made:
            h = eng.hash_to_g1_batch(D.msgs, D.dst)
            assert h[:64 * 4] == oracle.hash_to_g1_batch(D.msgs[:4], D.dst)
            made[id(D)] = (oracle.multi_miller_loop(h, D.pks, D.n),
                           oracle.multi_miller_loop(h + D.agg, D.pks + neg_g2(oracle.g2_generator()), D.n + 1))
        return made[id(D)]
    return get


# ---------------- aggregate_verify: per-key sums (aggregate_verify_grouped)
def test_aggregate_verify_few_pairs_one_wave_per_key(engines, few, oracle):
    """8 pairs over 3 keys: the grouped path whatever the keys, 3 + 1 sums on miller_wide_1p, one value per pair"""
    e = engines["default"]
    for label, pks, msgs, sig, keys in few.damaged():
        g0, p0 = e.aggregate_path_stats()
        got, rec = launches(e, lambda: e.aggregate_verify(pks, msgs, sig, few.dst), RECORDED)
        assert got is (label == "valid") and got is oracle.aggregate_verify(pks, msgs, sig, few.dst), label
        assert rec == record("miller_wide_1p", keys + 1, 1), label
        assert e.aggregate_path_stats() == (g0 + 1, p0), label


@pytest.mark.parametrize("name,kernel", [("tri", "miller_tri_1p"), ("lane", "miller_hpk1p")])
def test_aggregate_verify_repeated_keys(engines, repeated, oracle, name, kernel):
    """1024 pairs over 4 keys: 4 + 1 sums, a quad of lanes per pair or -- the launch is far below a round of waves -- one pair per
    lane: 5 values, three levels (two pairs per lane would leave 3 values, two levels)"""
    e = engines[name]
    bad = list(repeated.msgs); bad[500] = b"tampered"
    for msgs, want in ((repeated.msgs, True), (bad, False)):
        g0, p0 = e.aggregate_path_stats()
        got, rec = launches(e, lambda: e.aggregate_verify(repeated.pks, msgs, repeated.agg, repeated.dst), RECORDED)
        assert got is want
        assert rec == record(kernel, 5, 1) and rec["fp12_mul_pairs"] == 3
        assert e.aggregate_path_stats() == (g0 + 1, p0)
    assert oracle.aggregate_verify(repeated.pks, repeated.msgs, repeated.agg, repeated.dst) is True


def test_aggregate_verify_distinct_keys_pair_by_pair(engines, distinct, products):
    """1024 pairs over 1024 keys without the small forms: the grouped path declines, the 1025 pairs run two per lane on the
    variable-key loop, then the finish (its one partial carries the signature's pair: no Miller loop of its own)"""
    e = engines["lane"]
    assert e.aggregate_finish(products(distinct)[1], 1, None) is True      # the oracle's product, finished: the input is valid
    bad = list(distinct.msgs); bad[77] = b"tampered"
    for msgs, want in ((distinct.msgs, True), (bad, False)):
        g0, p0 = e.aggregate_path_stats()
        got, rec = launches(e, lambda: e.aggregate_verify(distinct.pks, msgs, distinct.agg, distinct.dst), RECORDED)
        assert got is want
        assert rec == record("miller_hpk2", 513, 0)
        assert e.aggregate_path_stats() == (g0, p0 + 1)


# ---------------- aggregate_partial, aggregate_partial_with_sig
@pytest.mark.parametrize("name", ENGINES)
def test_aggregate_partial_from_tables(engines, repeated, products, name):
    """1024 pairs over 4 keys: the keys' tables, two pairs per lane on every engine; the bytes are the oracle's product"""
    e = engines[name]
    D = repeated
    want, want_sig = products(D)
    got, rec = launches(e, lambda: e.aggregate_partial(D.pks, D.msgs, D.dst), RECORDED)
    assert got == (want, True)
    assert rec == record("miller_hpk2p", 512, 1)
    got, rec = launches(e, lambda: e.aggregate_partial_with_sig(D.pks, D.msgs, D.agg, D.dst), RECORDED)
    assert got == (want_sig, True, True)
    assert rec == record("miller_hpk2p", 513, 1)


@pytest.mark.parametrize("name", ENGINES)
def test_aggregate_partial_few_pairs(engines, few, products, name):
    """8 pairs: below 1024 no tables, the variable-key loop"""
    e = engines[name]
    D = few
    want, want_sig = products(D)
    got, rec = launches(e, lambda: e.aggregate_partial(D.pks, D.msgs, D.dst), RECORDED)
    assert got == (want, True)
    assert rec == record("miller_hpk2", 4, 0)
    got, rec = launches(e, lambda: e.aggregate_partial_with_sig(D.pks, D.msgs, D.agg, D.dst), RECORDED)
    assert got == (want_sig, True, True)
    assert rec == record("miller_hpk2", 5, 0)


# ---------------- aggregate_verify_prepared
@pytest.mark.parametrize("name", ENGINES)
def test_aggregate_verify_prepared_two_pairs_per_lane(engines, few, oracle, name):
    """5 pairs over a table of 3 keys (and, as entry 3, a key outside the subgroup): 5 + 1 pairs, two per lane on every engine"""
    e = engines[name]
    n = 5
    D = Pairs(e, n, 3, few.dst, 44)
    prep = e.g2_prepare_batch(b"".join(D.key_pool) + synth.NON_SUBGROUP_PK, 4)
    try:
        bad = list(D.msgs); bad[2] = b"tampered"
        for label, idx, msgs, sig in (("valid", D.idx, D.msgs, D.agg), ("message", D.idx, bad, D.agg), ("identity_sig", D.idx, D.msgs, IDENT1),
                                      ("outside_key", D.idx[:-1] + [3], D.msgs, D.agg)):
            got, rec = launches(e, lambda: e.aggregate_verify_prepared(prep, idx, msgs, sig, D.dst), RECORDED)
            pks = b"".join((D.key_pool + [synth.NON_SUBGROUP_PK])[k] for k in idx)
            assert got is (label == "valid") and got is oracle.aggregate_verify(pks, msgs, sig, D.dst), label
            assert rec == record("miller_hpk2p", 3, 0), label
    finally:
        prep.close()


# ---------------- aggregate_verify_batch_rlc: a second round never shares a lane between two slots
def test_aggregate_rlc_second_round_one_pair_per_lane(engines, M):
    """12 groups of 3 pairs over 8 keys, one wrong message, 4 segments, no wave or quad kernels: round 1 (9 slots) and round 2
    (36 slots) each run miller_hpk1p once -- a lane's value must belong to ONE segment slot, so never miller_hpk2p -- and the failed
    segment's groups go to the exact pipeline's own loop.  Round 1's product is a tree over 9 values; round 2's is segmented."""
    e = engines["lane"]
    n_g, bad = 12, 7
    D = Data(e, [3] * n_g, M.DEFAULT_DST, salt=45)
    D.flip_message(bad, 1)
    e.set_aggregate_rlc_segments(4)
    try:
        got, rec = launches(e, lambda: e.aggregate_verify_batch_rlc(*D.args(), SEED), RECORDED)
    finally:
        e.set_aggregate_rlc_segments(0)
    assert bits_of(got, n_g) == [g != bad for g in range(n_g)]
    assert got == e.aggregate_verify_batch(*D.args())
    assert rec == record("miller_hpk1p", 9, 1, miller_hpk1p=2, miller_hpk2r=1)

