"""What the tests of the built library share: the package as a fixture, the entry points include/blsbn254.h declares, and the
kernels' metadata and disassembly counts, read once per run through scripts/kernel_resources.py and scripts/isa_lint.py.
No GPU needed.  Nothing else under tests/ runs the binary tools itself."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "scripts") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "scripts"))

from abi_header import prototypes                                                                    # noqa: E402
from isa_lint import lint                                                                            # noqa: E402
from kernel_resources import demangled, instruction_counts, kernel_table, library_path_built, scratch_bytes       # noqa: E402,F401


@pytest.fixture(scope="module")
def M():
    import blsbn254_loader
    return blsbn254_loader.load()


def declared_symbols():
    return sorted(p.name for p in prototypes())


def lint_by_name(path):
    """isa_lint's counters per function, under the demangled name without parameters"""
    counts = lint(path)
    names = demangled(counts)
    return {names[sym]: c for sym, c in counts.items()}
