"""The built library contains the kernels of the wire-format aggregation and merge calls, and they are real code: the instruction
count that tests/test_kernel_sanity.py::test_no_degenerate_kernels applies to every kernel, and the scratch of the two scans
(the table of the square-root chain and nothing else), read from the gfx950 code objects through scripts/kernel_resources.py.
No GPU needed."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
KERNELS = ("k_ka_scan_wire", "k_kca_scan_wire", "k_g1p_to_wire")


def library():
    import blsbn254_loader
    M = blsbn254_loader.load()
    path = M.library_path()
    if not os.path.exists(path):
        __import__("bls_bn254_amd.build", fromlist=["x"]).build()
    return M, path


def test_wire_kernels_are_in_the_library_and_not_degenerate():
    _, path = library()
    from kernel_resources import code_objects
    tmp = tempfile.mkdtemp()
    sizes, scratch, spills = {}, {}, {}
    for idx, (data, off, size) in enumerate(code_objects(path)):
        co = os.path.join(tmp, "co_%d.o" % idx)
        open(co, "wb").write(data[off:off + size])
        notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True).stdout
        if not any(k in notes for k in KERNELS):
            continue
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s*(\S+)", blk).group(1)
            scratch[name] = int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk).group(1))
            spills[name] = int(re.search(r"\.vgpr_spill_count:\s*(\d+)", blk).group(1)) + int(re.search(r"\.sgpr_spill_count:\s*(\d+)", blk).group(1))
        dis = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                cur = m.group(1); sizes.setdefault(cur, 0)
            elif cur and re.match(r"^\s+[a-z_0-9]+", line):
                sizes[cur] += 1
    for k in KERNELS:
        names = [s for s in sizes if re.search(r"\d%s(?![a-z_0-9])" % k, s)]          # the mangled name: <length><name><parameters>
        assert len(names) == 1, (k, sorted(sizes))
        assert sizes[names[0]] >= 200, "suspiciously small kernel (undefined behaviour in the source?): %s %d" % (names[0], sizes[names[0]])
        assert spills[names[0]] == 0, (k, spills)
        if k != "k_g1p_to_wire":
            # the table of fp_pow_pm3_4 (14 field elements of 36 bytes) lives in scratch, and nothing else should
            assert 504 <= scratch[names[0]] <= 1024, (k, scratch)


def test_the_library_exports_the_wire_format_entry_points():
    M, _ = library()
    lib = M.load_library()
    for name in ("blsbn254_keyset_aggregate_checked_batch_compressed", "blsbn254_keyset_committee_aggregate_checked_batch_compressed",
                 "blsbn254_keyset_merge_checked_batch_compressed", "blsbn254_keyset_committee_merge_checked_batch_compressed",
                 "blsbn254_keyset_committee_fast_aggregate_verify_batch_compressed"):
        assert hasattr(lib, name), name
