"""GPU test (MI355X) of the four checked calls over a registered key set run against one another on ONE context: the checked
aggregation and the checked merge, over the registry and per committee, each on 64-byte and on 32-byte signatures.  Their host
state is one shared type (host_keyset_checked.hip), so what could go wrong is state that outlives a call: the fail list, the
per-entry messages, the downloaded bits, a buffer sized by an earlier call.  Every call of a fixed interleaving -- large, then
small, then large again -- must give what the same call gives on a fresh context of its own: outputs byte for byte, the same
four counts, the siblings' counts untouched.  The calls themselves are pinned to the oracle by their own test files."""
import pytest

from tests.gpu_support import eng, fresh_engine, M
from tests.keyset_support import as_args, chunks, com_args, compress_entries, compressed, Con, delta, keys_of, sign_all, sign_positions, ST_SHORT, World

pytestmark = pytest.mark.gpu
CALLS = {"agg": "keyset_aggregate", "cagg": "keyset_committee_aggregate", "mrg": "keyset_merge", "cmrg": "keyset_committee_merge"}
# per size: the groups' committees (0: one member, a row of one byte; 1, 3, 5: rows of 4, 5 and 17 bytes over a registry of 140
# keys, 17.5 bytes) and their entries.  Every size has a group that takes the fallback and succeeds (one wrong entry among honest
# ones), one that takes it and ends short (its only entry is wrong), an empty group and a group settled optimistically; the large
# size sends 12 + 6 + 1 entries to the fallback (its per-entry pass is cut by the 8-lane chunk), the small one 3 + 1
SHAPES = {"large": ([5, 3, 0, 1, 1], [12, 6, 1, 0, 4]), "small": ([3, 0, 1, 5], [3, 1, 0, 2])}
WRONG = {"large": {(0, 4), (1, 1), (2, 0)}, "small": {(0, 2), (1, 0)}}      # (group, entry) signed with another secret key
STATUS = {"large": bytes([0, 0, ST_SHORT, ST_SHORT, 0]), "small": bytes([0, ST_SHORT, ST_SHORT, 0])}
COUNTS = {"large": (1, 3, 19, 2), "small": (1, 2, 4, 2)}      # optimistic groups, fallback groups, entries verified there, short groups


@pytest.fixture(scope="module")
def W(eng, M):
    return World(eng, M)


def messages(size, n):
    """one message per group, of different lengths; the empty group's is empty"""
    return [b"" if not n[g] else (b"checked sequence %s %d " % (size.encode(), g)) * (1 + g % 3) for g in range(len(n))]


def wire_groups(eng, groups):
    """merge arguments [[(row, 64-byte signature)]] with the signatures compressed"""
    c = compressed(eng, b"".join(sig for cs in groups for _, sig in cs))
    it = iter(c[32 * t:32 * t + 32] for t in range(len(c) // 32))
    return [[(row, next(it)) for row, _ in cs] for cs in groups]


def arguments(eng, W, size):
    """(form, wire) -> the arguments of that call between the handle and the DST"""
    com, n = SHAPES[size]
    msgs = messages(size, n)
    # the collector's entries: positions spread over the committee's row words
    pos = [W.clean[c][::max(1, len(W.clean[c]) // max(k, 1))][:k] for c, k in zip(com, n)]
    assert [len(p) for p in pos] == n
    wrong = {(g, pos[g][j]) for g, j in WRONG[size]}
    ent = sign_positions(eng, W, com, [set(p) for p in pos], msgs, sk=lambda g, p: W.reg.sk[W.coms[com[g]][p]] + 1 if (g, p) in wrong else None)
    went = compress_entries(eng, ent)
    by_key = lambda entries: [{W.coms[c][p]: s for p, s in es.items()} for c, es in zip(com, entries)]
    # the intermediate node's contributions: disjoint key sets of its group's committee
    width = {5: 2, 3: 3, 0: 1, 1: 2}
    groups = [[Con(x, sk_delta=int((g, j) in WRONG[size]), good=(g, j) not in WRONG[size]) for j, x in enumerate(chunks(keys_of(W, c), [width[c]] * k))]
              for g, (c, k) in enumerate(zip(com, n))]
    sign_all(eng, W.reg, groups, msgs, W.dst)
    wide, per_com = as_args(groups), com_args(W.coms, com, groups)
    return {("agg", False): (by_key(ent), msgs), ("agg", True): (by_key(went), msgs),
            ("cagg", False): (com, ent, msgs), ("cagg", True): (com, went, msgs),
            ("mrg", False): (wide, msgs), ("mrg", True): (wire_groups(eng, wide), msgs),
            ("cmrg", False): (com, per_com, msgs), ("cmrg", True): (com, wire_groups(eng, per_com), msgs)}


def stats(e):
    return {form: getattr(e, name + "_stats")() for form, name in CALLS.items()}


def run(e, ks, W, args, form, wire):
    """(the call's result, what it added to the four forms' counts)"""
    s0 = stats(e)
    res = getattr(e, CALLS[form] + "_checked_batch" + ("_compressed" if wire else ""))(ks, *args[form, wire], W.dst)
    s1 = stats(e)
    return res, {f: tuple(delta(s1[f], s0[f]).values()) for f in CALLS}


def test_interleaved_calls_on_one_context(eng, M, W, monkeypatch):
    args = {size: arguments(eng, W, size) for size in SHAPES}
    # large: every form once, the encodings alternating; small, then large again: all eight calls
    eight = [(form, wire) for wire in (False, True) for form in CALLS]
    sequence = [("large", form, g % 2 == 1) for g, form in enumerate(CALLS)]
    sequence += [("small", form, wire) for form, wire in eight] + [("large", form, wire) for form, wire in reversed(eight)]
    fresh = {}
    for size in SHAPES:
        for form, wire in eight:
            e = fresh_engine(M, monkeypatch, "8")
            try:
                ks = W.keyset(M, e, False)
                fresh[size, form, wire] = res, added = run(e, ks, W, args[size], form, wire)
                ks.close()
            finally:
                e.close()
            # the case is what the table above says: statuses, counts, and nothing on the siblings
            assert res[-1] == STATUS[size] and added == {f: COUNTS[size] if f == form else (0, 0, 0, 0) for f in CALLS}, (size, form, wire)
            if form in ("mrg", "cmrg"):
                assert res[2] == [[(g, j) not in WRONG[size] for j in range(k)] for g, k in enumerate(SHAPES[size][1])], (size, form, wire)
    for wire in (False, True):                                # the committee forms agree with the full-width ones on signatures
        assert fresh["large", "cagg", wire][0][0] == fresh["large", "agg", wire][0][0] and fresh["large", "cmrg", wire][0][0] == fresh["large", "mrg", wire][0][0]
    e = fresh_engine(M, monkeypatch, "8")
    try:
        ks = W.keyset(M, e, False)
        for step, (size, form, wire) in enumerate(sequence):
            assert run(e, ks, W, args[size], form, wire) == fresh[size, form, wire], "step %d: %s %s, compressed %s" % (step, size, form, wire)
        ks.close()
    finally:
        e.close()
