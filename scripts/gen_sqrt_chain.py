"""Addition chain for the ONE exponent of the hash's square-root power, a^((p-3)/4) (curve.h svdw_g1_frac), as a table for
fp_pow_pm3_4 (fp29.h): odd powers a^1, a^3, ..., a^(2 TAB - 1) first (one squaring + TAB - 1 products), then a list of
(squarings, table index) steps fixed at generation time -- sliding windows over the bits of this exponent, so the device runs a
table-driven loop with uniform control flow and never looks at exponent bits.

Searches the window width and the table size (windows are cut so that their value stays below 2 TAB), keeps the cheapest in
products, checks it with Python integers and prints the macro for fp29.h.  --check parses the macro in fp29.h and checks THAT.
Usage: python scripts/gen_sqrt_chain.py [--check]"""
import os
import random
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
E = (P - 3) // 4


def windows(e, width, max_odd):
    """Left-to-right sliding windows: [(squarings before the product, odd value)], first entry = the leading window (0 squarings)."""
    bits = bin(e)[2:]
    steps, i, pending = [], 0, 0
    n = len(bits)
    while i < n:
        if bits[i] == "0":
            pending += 1; i += 1
            continue
        j = min(n, i + width)
        while True:                                   # longest window ending in a one whose value fits the table
            while bits[j - 1] == "0":
                j -= 1
            if int(bits[i:j], 2) <= max_odd:
                break
            j -= 1
        steps.append((pending + (j - i), int(bits[i:j], 2)))
        pending = 0
        i = j
    first = steps[0]
    steps[0] = (0, first[1])
    return steps, pending                             # pending: squarings after the last product


def cost(steps, tail):
    tab = (max(v for _, v in steps) + 1) // 2
    muls = (tab - 1) + (len(steps) - 1)
    sqrs = (1 if tab > 1 else 0) + sum(s for s, _ in steps) + tail
    return muls, sqrs, tab


def run(a, steps, tail, p=P):
    tab_n = (max(v for _, v in steps) + 1) // 2
    a2 = a * a % p
    tab = [a % p]
    for _ in range(tab_n - 1):
        tab.append(tab[-1] * a2 % p)
    r = tab[(steps[0][1] - 1) // 2]
    for s, v in steps[1:]:
        for _ in range(s):
            r = r * r % p
        r = r * tab[(v - 1) // 2] % p
    for _ in range(tail):
        r = r * r % p
    return r


def check(steps, tail):
    assert sum(v << 0 for _, v in steps) >= 0
    acc = 0
    for s, v in steps:                                # the chain as an integer: it must BE the exponent
        acc = (acc << s) + v
    acc <<= tail
    assert acc == E, "chain does not reach (p-3)/4"
    rnd = random.Random(7)
    for a in [0, 1, P - 1] + [rnd.randrange(P) for _ in range(200)]:
        assert run(a, steps, tail) == pow(a, E, P), a


def search():
    best = None
    for width in range(3, 9):
        for max_odd in range(3, 1 << width, 2):
            steps, tail = windows(E, width, max_odd)
            c = cost(steps, tail)
            if best is None or (c[0], c[1]) < (best[0][0], best[0][1]):
                best = (c, width, max_odd, steps, tail)
    return best


def parse_header():
    src = open(os.path.join(ROOT, "bls-bn254_amd", "csrc", "fp29.h")).read()
    m = re.search(r"#define BN_PM3_4_CHAIN \{(.*?)\}\s*\n", src.replace("\\\n", " "), re.S)
    pairs = re.findall(r"\{\s*(\d+)\s*,\s*(\d+)\s*\}", m.group(1))
    first = int(re.search(r"BN_PM3_4_FIRST = (\d+)", src).group(1))
    steps = [(0, 2 * first + 1)] + [(int(s), 2 * int(i) + 1) for s, i in pairs]
    return steps, 0


def main():
    if "--check" in sys.argv:
        steps, tail = parse_header()
        check(steps, tail)
        print("fp29.h chain ok: %d products, %d squarings, table of %d odd powers" % cost(steps, tail))
        return
    (muls, sqrs, tab), width, max_odd, steps, tail = search()
    assert tail == 0                                  # the exponent is odd
    check(steps, tail)
    print("// window width %d, odd powers up to %d: %d products (%d table + %d chain), %d squarings; 4-bit fixed windows: 77 + 252"
          % (width, max_odd, muls, tab - 1, len(steps) - 1, sqrs))
    print("constexpr int BN_PM3_4_TAB = %d, BN_PM3_4_FIRST = %d, BN_PM3_4_LEN = %d;" % (tab, (steps[0][1] - 1) // 2, len(steps) - 1))
    body = ", ".join("{%d, %d}" % (s, (v - 1) // 2) for s, v in steps[1:])
    print("#define BN_PM3_4_CHAIN {%s}" % body)


if __name__ == "__main__":
    main()
