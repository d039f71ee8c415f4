"""The one reader of include/blsbn254.h: every entry point's name, C return type and ordered parameters.  The Rust extern block
(integration/rust/gen_ffi.py), the Python prototype table (scripts/gen_abi.py) and the tests (tests/library_support.py) all
take the C ABI from here, so none of them can drift from the header or from each other."""
import collections
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "blsbn254.h")

Param = collections.namedtuple("Param", "name ctype is_array")
Prototype = collections.namedtuple("Prototype", "name ret params")


def prototypes(header=HEADER):
    """[Prototype(name, C return type, (Param(name, C type, is_array), ..))] in the header's order.  The types are the
    header's tokens joined by one space (`const uint8_t*`, `blsbn254_ctx**`); a `T name[64]` parameter has C type `T` and
    is_array set."""
    s = open(header).read()
    s = re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    s = re.sub(r"//.*", "", s)
    out = []
    for ret, name, args in re.findall(r"\n\s*([A-Za-z_][\w\s\*]*?)\b(blsbn254_\w+)\s*\(([^;{]*?)\)\s*;", s):
        params = []
        for a in args.split(","):
            m = re.match(r"^(.*?)(\w+)\s*(\[\d*\])?$", " ".join(a.split()))
            params.append(Param(m.group(2), m.group(1).strip(), m.group(3) is not None))
        out.append(Prototype(name, " ".join(ret.split()), tuple(params)))
    return out
