"""CPU-only: the operations trimmed from the verify hot path, run from the device headers on the host with -DBN_CHECK
(tests/hostsim/op_trim_host.cpp: every multiply asserts the lazy-limb interval discipline, so a run that returns has passed the
interval checker on every function it went through) and counted by the operation counters of scripts/op_trim_counts.py against
the committed profiles/op_trim.json:
  * the prepared Miller loop, whose first step is left as it was (DESIGN section 5 says why): the parent's counts, and the bytes
    after the final exponentiation those of the parent (tests/golden/op_trim_parent_fe.json) and of the oracle;
  * the verify form of the last final-exponentiation step: one dense Fp12 product fewer, the same verdict as fp12_is_one of the
    full step;
  * the t^x chain table reaches x (Python integers on the table itself);
  * the fixed chain of the hash's square-root power equals pow(a, (p - 3) / 4, p);
  * the constant SHA-256 state of expand_message_xmd is a Python compression of the zero block.
A test tool; the product has no CPU path."""
import ctypes
import json
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
GT_ONE = (1).to_bytes(32, "big") + bytes(352)
PRODUCTS = ("fp_mul", "fp_sqr", "fp_dot2")
COUNTERS = PRODUCTS + ("fp_norm", "fp_lc_passes", "fp_lc_terms")
MILLER = "miller_loop_prepared_unit (k_miller_prepared)"
CHAIN = "cyclotomic_exp_x_chain (one t^x launch)"
H3_VERDICT = "fe_h3_loop, 7 steps + fe_h3_verdict (k_fe_h3, verify modes)"
H3_FULL = "fe_h3_loop, 8 steps + fp12_is_one (k_fe_h3, Gt modes)"
DENSE = "fp12_mul_mem (one dense product)"
HASH = "lane_hash_to_g1_proj (k_hash_to_g1), 32-byte message"


@pytest.fixture(scope="module")
def hs():
    import op_trim_counts
    return op_trim_counts.load()


@pytest.fixture(scope="module")
def committed():
    return json.load(open(os.path.join(ROOT, "profiles", "op_trim.json")))


@pytest.fixture(scope="module")
def measured(hs, oracle):
    import op_trim_counts
    return op_trim_counts.measure(hs, oracle)


def test_counts_are_the_committed_ones(measured, committed):
    assert measured == committed["after"]


def test_miller_loop_count_is_the_parents(measured, committed):
    """The first-iteration peel of the prepared Miller loop is NOT part of this change: the loop executes what
    the parent's executed, counter by counter."""
    assert measured[MILLER] == committed["before"][MILLER]


def test_verify_h3_runs_one_dense_product_fewer(measured, committed):
    full, verdict, dense = measured[H3_FULL], measured[H3_VERDICT], measured[DENSE]
    assert committed["before"][H3_VERDICT] == full            # the parent ran the full step in every mode
    assert dense["fp_dot2"] == 36 and dense["fp_mul"] == dense["fp_sqr"] == 0          # 18 Fp2 products
    assert full["fp_dot2"] - verdict["fp_dot2"] == dense["fp_dot2"]
    assert full["fp_sqr"] == verdict["fp_sqr"] == 0
    # the comparison canonicalises 24 coefficients (one product with the Montgomery one each) where fp12_is_one canonicalised 12
    assert verdict["fp_mul"] - full["fp_mul"] == 12
    assert verdict["executed_mads"] < full["executed_mads"]


def test_expx_chain_table_reaches_x(hs, pyref, measured, committed):
    """The interpreter of cyclotomic_exp_x_chain on exponents: slot 0 holds f, `load` replaces the running value, `sq` doubles
    it, `mul` adds a slot, `store` parks it, `cstore` parks its conjugate (the negative)."""
    raw = (ctypes.c_int8 * 320)()
    nslots = ctypes.c_int()
    n = hs.hs_ot_chain_table(raw, ctypes.byref(nslots))
    slots = {0: 1}
    r, sq, mul = 1, 0, 0
    for k in range(n):
        load, s, m, store, cstore = raw[5 * k:5 * k + 5]
        if load >= 0:
            r = slots[load]
        r <<= s
        sq += s
        if m >= 0:
            r += slots[m]
            mul += 1
        if store >= 0:
            slots[store] = r
        if cstore >= 0:
            slots[cstore] = -r
    print("t^x chain: %d squarings + %d products, %d parked powers" % (sq, mul, len(slots)))
    assert r == pyref.X
    assert len(slots) <= nslots.value and max(slots) < nslots.value
    assert mul <= 12 and sq <= 64 and nslots.value <= 5       # the chain before: 13 products + 62 squarings, 5 slots
    # one product fewer is one dense Fp12 product fewer per launch, squarings as before
    before, after, dense = committed["before"][CHAIN], measured[CHAIN], measured[DENSE]
    assert before["fp_dot2"] - after["fp_dot2"] == (13 - mul) * dense["fp_dot2"] and (13 - mul) >= 1
    assert before["fp_mul"] == after["fp_mul"] and sq == 62   # the cyclotomic squarings (their count is in fp_mul) did not change


def test_sqrt_chain_equals_the_power(hs, pyref, measured):
    P = pyref.P
    rnd = random.Random(5)
    out, win = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    c1, c2 = (ctypes.c_double * 7)(), (ctypes.c_double * 7)()
    for a in [0, 1, P - 1] + [rnd.randrange(P) for _ in range(200)]:
        hs.hs_ot_pow_pm3_4(a.to_bytes(32, "big"), out, win, c1, c2)
        want = pow(a, (P - 3) // 4, P).to_bytes(32, "big")
        assert out.raw == want and win.raw == want, a
    chain, window = measured["fp_pow_pm3_4 (fixed chain)"], measured["fp_pow, 4-bit fixed windows"]
    print("square-root power: %d products + %d squarings (4-bit windows: %d + %d)" % (chain["fp_mul"], chain["fp_sqr"], window["fp_mul"], window["fp_sqr"]))
    assert window["fp_mul"] - chain["fp_mul"] >= 20 and chain["fp_sqr"] <= window["fp_sqr"]
    import gen_sqrt_chain
    steps, tail = gen_sqrt_chain.parse_header()                # the table in fp29.h IS the exponent, as an integer
    gen_sqrt_chain.check(steps, tail)
    assert gen_sqrt_chain.cost(steps, tail)[:2] == (chain["fp_mul"], chain["fp_sqr"])


def test_hash_runs_two_shorter_powers_and_one_compression_fewer(measured, committed):
    before, after = committed["before"][HASH], measured[HASH]
    chain, window = measured["fp_pow_pm3_4 (fixed chain)"], measured["fp_pow, 4-bit fixed windows"]
    assert before["fp_mul"] - after["fp_mul"] == 2 * (window["fp_mul"] - chain["fp_mul"])
    assert before["fp_sqr"] - after["fp_sqr"] == 2 * (window["fp_sqr"] - chain["fp_sqr"])
    assert before["sha256_blocks"] - after["sha256_blocks"] == 1


def test_sha_zero_block_state(hs):
    import sha256_zero_block_state as Z
    import hashlib
    for m in (b"", b"abc", bytes(64), bytes(range(200))):     # the Python compression itself, against known digests
        assert Z.sha256(m) == hashlib.sha256(m).digest()
    got = (ctypes.c_uint32 * 8)()
    hs.hs_ot_sha_zpad_state(got)
    assert list(got) == Z.zero_block_state()


def test_hash_to_g1_equals_the_oracle(hs, oracle):
    """expand_message_xmd from the constant state and the fixed chain in the map: message lengths on both sides of the block
    boundaries of b_0 (64 + len + 3 + len(dst) + 1 bytes before the padding), a one-byte and a 255-byte DST."""
    pt = ctypes.create_string_buffer(64)
    c = (ctypes.c_double * 7)()
    for dst in (b"D", bytes(range(1, 256))):
        msgs = [bytes((7 * i + k) & 255 for k in range(n)) for i, n in enumerate((0, 1, 32, 55, 56, 64, 200))]
        want = oracle.hash_to_g1_batch(msgs, dst)
        for i, m in enumerate(msgs):
            hs.hs_ot_hash(m, len(m), dst, len(dst), pt, c)
            assert pt.raw == want[64 * i:64 * i + 64], (len(m), len(dst))


def test_fe_bytes_are_the_parents(hs, oracle, pyref):
    """The prepared Miller loop followed by the full final_exponentiation: byte-identical to what the parent's loop gave on the
    same inputs (recorded from the parent's build), and to the oracle's final exponentiation of the textbook Miller value."""
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "op_trim_parent_fe.json")))
    neg_g2 = pyref.g2_to_bytes(pyref.g2_neg(pyref.G2_GEN))
    gt = ctypes.create_string_buffer(384)
    c = (ctypes.c_double * 7)()
    ones = 0
    for case in doc["cases"]:
        sig, h, pk = (bytes.fromhex(case[k]) for k in ("sig", "h", "pk"))
        assert hs.hs_ot_miller(sig, h, pk, case["z"], gt, c) == 0
        assert gt.raw == bytes.fromhex(case["fe"])
        assert gt.raw == oracle.final_exponentiation(oracle.multi_miller_loop(sig + h, neg_g2 + pk, 2), 1)
        ones += gt.raw == GT_ONE
    assert ones == len(doc["cases"]) // 2


def test_h3_verdict_equals_is_one_of_the_full_step(hs, oracle, pyref):
    import op_trim_counts
    sk = 0x1234567
    pk = oracle.sk_to_pk(sk)
    dst = b"D"
    msg = b"op trim"
    sig = oracle.sign(sk, msg, dst)
    neg_g2 = pyref.g2_to_bytes(pyref.g2_neg(pyref.G2_GEN))

    def miller(m):
        return oracle.multi_miller_loop(sig + oracle.hash_to_g1_batch([m], dst), neg_g2 + pk, 2)
    v, full, *_ = op_trim_counts.h3(hs, miller(msg))                          # a valid tuple
    assert v == full == 1
    v, full, *_ = op_trim_counts.h3(hs, miller(b"op trin"))                   # a corrupted message
    assert v == full == 0
    for coeff in (0, 5, 6, 11):                                               # the two sides differ in one coefficient
        v, full, *_ = op_trim_counts.h3(hs, miller(msg), coeff)
        assert v == full == 0, coeff
    # f = 0: every phase value is zero and the two sides agree; neither form may say "one"
    assert hs.hs_ot_h3_zero() == 0
