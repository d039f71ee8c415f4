"""Executed operations per tuple of the four phases that the operation trim touches -- the prepared Miller loop, one t^x chain,
the verify form of the last final-exponentiation step and one hash -- counted like scripts/executed_mads.py does: the DEVICE
headers run on the host (tests/hostsim/op_trim_host.cpp, -DBN_CHECK) with the operation counters on; the counts are data
independent.  Writes the "after" section of profiles/op_trim.json and leaves its other sections (the parent's counts under
"before", the timings) as they are; profiles/r03_executed_mads.json, which bench.py reads, is not touched.
Usage: python scripts/op_trim_counts.py [--print-only]"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIM = os.path.join(ROOT, "tests", "hostsim")
PATH = os.path.join(ROOT, "profiles", "op_trim.json")
NAMES = ("fp_mul", "fp_sqr", "fp_dot2", "fp_norm", "fp_lc_passes", "fp_lc_terms", "sha256_blocks")
DST = b"D"
MSG = bytes(range(32))                       # a 32-byte message, as the benchmark's


def load():
    so = os.path.join(SIM, "libop_trim.so")
    csrc = os.path.join(ROOT, "bls-bn254_amd", "csrc")
    src = [os.path.join(SIM, "op_trim_host.cpp")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(p) > os.path.getmtime(so) for p in src):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-DBN_CHECK", "-fPIC", "-shared", "-pthread", "-o", so, os.path.join(SIM, "op_trim_host.cpp")])
    return ctypes.CDLL(so)


def counts():
    return (ctypes.c_double * 7)()


def entry(c):
    e = {n: int(v) for n, v in zip(NAMES, c)}
    e["executed_mads"] = 162 * e["fp_mul"] + 126 * e["fp_sqr"] + 243 * e["fp_dot2"] + 9 * e["fp_lc_terms"]
    return e


def h3(hs, f, coeff=-1):
    """(verdict form, full form, counts of each, counts of one dense product) of the last step on the Miller value f"""
    v, full = ctypes.c_int(), ctypes.c_int()
    cv, cf, cd = counts(), counts(), counts()
    assert hs.hs_ot_h3(f, coeff, ctypes.byref(v), ctypes.byref(full), cv, cf, cd) == 0, "fe_h3_loop differs from fe_h3"
    return v.value, full.value, entry(cv), entry(cf), entry(cd)


def measure(hs, O):
    """The counts of the tree as it stands."""
    from oracle.pyref import bn254 as B
    from tests import synth
    sk = synth.sk_of(3)
    pk = O.sk_to_pk(sk)
    h = O.hash_to_g1_batch([MSG], DST)
    sig = O.sign(sk, MSG, DST)
    gt = ctypes.create_string_buffer(384)
    out = {}
    c = counts()
    assert hs.hs_ot_miller(sig, h, pk, 1, gt, c) == 0
    out["miller_loop_prepared_unit (k_miller_prepared)"] = entry(c)
    f = O.multi_miller_loop(sig + h, B.g2_to_bytes(B.g2_neg(B.G2_GEN)) + pk, 2)
    c = counts()
    assert hs.hs_ot_expx(f, c) == 1
    out["cyclotomic_exp_x_chain (one t^x launch)"] = entry(c)
    v, full, cv, cf, cd = h3(hs, f)
    assert v == full == 1
    out["fe_h3_loop, 7 steps + fe_h3_verdict (k_fe_h3, verify modes)"] = cv
    out["fe_h3_loop, 8 steps + fp12_is_one (k_fe_h3, Gt modes)"] = cf
    out["fp12_mul_mem (one dense product)"] = cd
    c = counts()
    pt = ctypes.create_string_buffer(64)
    hs.hs_ot_hash(MSG, len(MSG), DST, len(DST), pt, c)
    assert pt.raw == h
    out["lane_hash_to_g1_proj (k_hash_to_g1), 32-byte message"] = entry(c)
    a = (5).to_bytes(32, "big")
    r1, r2 = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    c1, c2 = counts(), counts()
    hs.hs_ot_pow_pm3_4(a, r1, r2, c1, c2)
    assert r1.raw == r2.raw
    out["fp_pow_pm3_4 (fixed chain)"] = entry(c1)
    out["fp_pow, 4-bit fixed windows"] = entry(c2)
    return out


def main():
    from oracle import oracle as O
    O.build()
    after = measure(load(), O)
    print(json.dumps(after, indent=1))
    if "--print-only" in sys.argv:
        return
    doc = json.load(open(PATH)) if os.path.exists(PATH) else {}
    doc["how"] = ("tests/hostsim/op_trim_host.cpp: the device headers run on the host with operation counters (data independent); "
                  "MADs = 162 fp_mul + 126 fp_sqr + 243 fp_dot2 + 9 fp_lc terms")
    doc["after"] = after
    json.dump(doc, open(PATH, "w"), indent=1)


if __name__ == "__main__":
    main()
