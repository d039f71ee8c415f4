"""CPU-only: the test modules stay readable on their own.  What two of them share lives in a support module (hostsim_build,
library_support, gpu_support, helpers, fp12_cases, keyset_support, threshold_support), never in another test module, and only the support
modules run the compiler of the host-side programs or the binary tools that read the library's code objects."""
import glob
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
TOOLS = ("g++", "llvm-readelf", "llvm-objdump")


def test_test_modules_import_no_test_module_and_run_no_build_tool():
    paths = [p for p in sorted(glob.glob(os.path.join(HERE, "test_*.py"))) if p != os.path.abspath(__file__)]      # (this one names the tools)
    assert len(paths) >= 60
    for path in paths:
        text = open(path).read()
        name = os.path.basename(path)
        assert not re.search(r"^\s*(from\s+tests\.test_\w+\s+import|import\s+tests\.test_\w+|from\s+tests\s+import\s+test_\w+)", text, re.M), name
        for tool in TOOLS:
            assert tool not in text, (name, tool)
