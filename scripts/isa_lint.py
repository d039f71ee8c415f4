"""Static checks of the built kernels for the code-generation accidents that cost this project time (each once, each invisible to
the tests): per kernel the number of read-first-lane loops (a buffer descriptor or scalar offset that reached a load through
vector registers: every access is serialised), flat accesses (an LDS or scratch address that lost its address space), the
scratch bytes per lane (spilled registers) and the instruction count.  Usage: python scripts/isa_lint.py [lib.so | obj.o ...]
-> one line per kernel; tests/test_kernel_sanity.py asserts limits on the kernels of the hot path."""
import collections
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import cached, demangled, disassembly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lint(path):
    """{symbol: Counter(total, readfirstlane, waterfall_loops, flat)} for every function symbol of the gfx950 code objects"""
    return cached("lint", path, _lint)


def _lint(path):
    out = {}
    for dis in disassembly(path):
        cur = None
        prev = ""
        for line in open(dis):
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                cur = out.setdefault(m.group(1), collections.Counter())
                continue
            t = line.strip().split()
            if not t or cur is None:
                continue
            op = t[0]
            cur["total"] += 1
            if op == "v_readfirstlane_b32":
                cur["readfirstlane"] += 1
            if op == "s_and_saveexec_b64" and prev.startswith(("v_cmp_eq", "s_and_b64", "s_nop")):
                cur["waterfall_loops"] += 1
            if op.startswith(("flat_load", "flat_store")):
                cur["flat"] += 1
            prev = op
    return out


def main():
    paths = sys.argv[1:] or [os.path.join(ROOT, "bls-bn254_amd", "libblsbn254_hip.so")]
    print("%-44s %8s %8s %8s %6s" % ("symbol", "instrs", "rfl", "wf-loops", "flat"))
    for p in paths:
        counts = lint(p)
        short = demangled(counts)
        for name, c in sorted(counts.items()):
            print("%-44s %8d %8d %8d %6d" % (short[name][:44], c["total"], c["readfirstlane"], c["waterfall_loops"], c["flat"]))


if __name__ == "__main__":
    main()
