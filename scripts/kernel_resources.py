"""Per-kernel resource usage of the built library (registers, spills, scratch, LDS), read from the code objects'
AMDGPU metadata notes -- no GPU and no recompilation needed.  Usage: python scripts/kernel_resources.py [lib.so]

The one reader of the library's gfx950 code objects: kernel_table() and instruction_counts() are what the tests assert on,
disassembly() is what scripts/isa_lint.py counts in.  Each is computed once per process and file (path, modification time, size)."""
import atexit
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
FIELDS = ("vgpr", "agpr", "vgpr_spills", "sgpr_spills", "scratch", "lds")
_cache = {}
_tmp = []


def code_objects(path):
    """(offset, size) of every gfx950 code object inside the clang offload bundles of a fat binary"""
    data = open(path, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    out = []
    pos = data.find(magic)
    while pos >= 0:
        n = int.from_bytes(data[pos + 24:pos + 32], "little")
        q = pos + 32
        for _ in range(n):
            off, size, tl = (int.from_bytes(data[q + 8 * k:q + 8 * k + 8], "little") for k in range(3))
            triple = data[q + 24:q + 24 + tl].decode()
            q += 24 + tl
            if "gfx950" in triple and size:
                out.append((data, pos + off, size))
        pos = data.find(magic, pos + 24)
    return out


def cached(what, path, make):
    st = os.stat(path)
    key = (what, os.path.abspath(path), st.st_mtime_ns, st.st_size)
    if key not in _cache:
        _cache[key] = make(path)
    return _cache[key]


def _workdir():
    if not _tmp:
        _tmp.append(tempfile.mkdtemp(prefix="code_objects_"))
        atexit.register(shutil.rmtree, _tmp[0], ignore_errors=True)
    return tempfile.mkdtemp(dir=_tmp[0])


def _extract(path):
    tmp, out = _workdir(), []
    for idx, (data, off, size) in enumerate(code_objects(path)):
        out.append(os.path.join(tmp, "co_%d.o" % idx))
        with open(out[-1], "wb") as f:
            f.write(data[off:off + size])
    return out


def extracted(path):
    """the gfx950 code objects of a fat binary as files of their own, in the order of code_objects()"""
    return cached("extract", path, _extract)


def _disassemble(path):
    out = []
    for co in extracted(path):
        out.append(co + ".s")
        with open(out[-1], "w") as f:
            subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", co], stdout=f, check=True)
    return out


def disassembly(path):
    """one text file per code object: its disassembly without the raw instruction words"""
    return cached("disassemble", path, _disassemble)


def demangled(names):
    """{name: the function's name without its parameters}, through one c++filt process"""
    names = sorted(set(names))
    mangled = [n for n in names if n.startswith("_Z")]
    out = {n: n for n in names}
    if mangled:
        text = subprocess.run(["c++filt"], input="\n".join(mangled) + "\n", capture_output=True, text=True, check=True).stdout
        out.update((n, d.split("(")[0].strip()) for n, d in zip(mangled, text.splitlines()))
    return out


def _kernel_table(path):
    rows = []
    for idx, co in enumerate(extracted(path)):
        notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            g = lambda k: int(re.search(r"\.%s:\s*(\d+)" % k, blk).group(1))
            rows.append({"symbol": re.search(r"\.name:\s*(\S+)", blk).group(1), "code_object": idx,
                         "vgpr": g("vgpr_count"), "agpr": int(blk.split("\n")[0]), "vgpr_spills": g("vgpr_spill_count"),
                         "sgpr_spills": g("sgpr_spill_count"), "scratch": g("private_segment_fixed_size"), "lds": g("group_segment_fixed_size")})
    names = demangled(r["symbol"] for r in rows)
    for r in rows:
        r["name"] = names[r["symbol"]]
    return rows


def kernel_table(path):
    """one dict per kernel: name (demangled, without parameters), symbol, code_object and FIELDS: registers, spill counts,
    scratch bytes per lane, LDS bytes"""
    return cached("kernels", path, _kernel_table)


def _instruction_counts(path):
    sizes = {}
    for s in disassembly(path):
        cur = None
        with open(s) as f:
            for line in f:
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    cur = m.group(1); sizes.setdefault(cur, 0)
                elif cur and re.match(r"^\s+[a-z_0-9]+", line):
                    sizes[cur] += 1
    return sizes


def instruction_counts(path):
    """{symbol: instructions} over every function symbol of the code objects"""
    return cached("instructions", path, _instruction_counts)


def library_path_built():
    """the package's library, built first when the file is missing"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import blsbn254_loader
    path = blsbn254_loader.load().library_path()
    if not os.path.exists(path):
        __import__("bls_bn254_amd.build", fromlist=["x"]).build()
    return path


def scratch_bytes(path=None):
    """{kernel name: scratch bytes per lane}"""
    return {r["name"]: r["scratch"] for r in kernel_table(path or library_path_built())}


def main():
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "bls-bn254_amd", "libblsbn254_hip.so")
    print("%-28s %5s %5s %7s %7s %9s %8s" % ("kernel", "vgpr", "agpr", "v-spill", "s-spill", "scratch B", "LDS B"))
    for r in sorted(set((r["name"],) + tuple(str(r[k]) for k in FIELDS) for r in kernel_table(lib))):
        print("%-28s %5s %5s %7s %7s %9s %8s" % r)


if __name__ == "__main__":
    main()
