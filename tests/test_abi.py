"""CPU-only: the C-ABI library loads, exports every symbol include/blsbn254.h declares, and refuses to
run without a gfx950 device (no CPU fallback)."""
import ctypes
import os
import re

import pytest

from tests.library_support import M, declared_symbols, library_path_built, prototypes  # noqa: F401 (M is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_surveyed_entry_points():
    syms = declared_symbols()
    for want in ("blsbn254_ctx_create", "blsbn254_ctx_destroy", "blsbn254_pairing_batch", "blsbn254_multi_miller_loop",
                 "blsbn254_final_exponentiation", "blsbn254_hash_to_g1_batch", "blsbn254_hash_to_g2_batch",
                 "blsbn254_g1_check_batch", "blsbn254_g2_check_batch", "blsbn254_verify_batch", "blsbn254_aggregate_verify",
                 "blsbn254_aggregate_sigs", "blsbn254_threshold_combine"):
        assert want in syms


def test_rust_shim_extern_block_matches_the_header():
    """integration/rust/ffi.rs is generated from include/blsbn254.h; the committed copy must be current and must
    declare every entry point exactly once (the reference-side binding)."""
    import subprocess
    import sys
    gen = os.path.join(ROOT, "integration", "rust", "gen_ffi.py")
    assert subprocess.call([sys.executable, gen, "--check"]) == 0, "run python integration/rust/gen_ffi.py"
    ffi = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    assert sorted(re.findall(r"pub fn (blsbn254_[a-z0-9_]+)\(", ffi)) == declared_symbols()
    shim = open(os.path.join(ROOT, "integration", "rust", "gpu.rs")).read()
    for used in set(re.findall(r"ffi::(blsbn254_[a-z0-9_]+)", shim)):
        assert used in declared_symbols()


def test_python_prototype_table_matches_the_header():
    """bls-bn254_amd/_abi.py is generated from include/blsbn254.h; the committed copy must be current."""
    import subprocess
    import sys
    gen = os.path.join(ROOT, "scripts", "gen_abi.py")
    assert subprocess.call([sys.executable, gen, "--check"]) == 0, "run python scripts/gen_abi.py"


def test_generator_refuses_a_type_it_does_not_know():
    import gen_abi                                           # scripts/ is on the path through tests.library_support
    assert gen_abi.arg_type("const uint8_t* const*", False) == gen_abi.arg_type("uint64_t", True) == "c_void_p"
    assert gen_abi.ret_type("blsbn254_ctx*") == "c_void_p" and gen_abi.ret_type("void") is None
    for bad in (lambda: gen_abi.arg_type("double", False), lambda: gen_abi.arg_type("uint64_t", False), lambda: gen_abi.ret_type("double")):
        with pytest.raises(SystemExit):
            bad()


def test_every_entry_point_has_the_headers_prototype(M):
    """load_library() sets argtypes and restype of every declared entry point, and nothing else has to: the calls below run
    with no restype or wrapper of their own."""
    lib = M.load_library()
    by_value = {"size_t": ctypes.c_size_t, "int": ctypes.c_int}
    returns = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p, "void": None}
    protos = prototypes()
    assert sorted(p.name for p in protos) == declared_symbols()
    for p in protos:
        fn = getattr(lib, p.name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(p.params), p.name
        for t, q in zip(fn.argtypes, p.params):
            assert t is (ctypes.c_void_p if q.is_array or q.ctype.endswith("*") else by_value[q.ctype]), (p.name, q.name)
        assert fn.restype is (returns[p.ret] if p.ret in returns else ctypes.c_void_p), p.name
    for count in (lib.blsbn254_keyset_count, lib.blsbn254_g2prepared_count, lib.blsbn254_keyset_committee_count):
        got = count(None)
        assert type(got) is int and got == 0
    assert type(lib.blsbn254_strerror(1)) is bytes
    with pytest.raises(TypeError):
        lib.blsbn254_g1_check_batch(None, None, 0)           # one argument too few


def test_a_library_without_a_declared_entry_point_is_refused_by_name(M, oracle, monkeypatch):
    """BLSBN254_LIB selects another build of the library; one that lacks an entry point of the header does not load (the
    oracle's shared library stands in for such a build)."""
    oracle.lib()
    monkeypatch.setattr(M.engine, "_lib", None)
    monkeypatch.setenv("BLSBN254_LIB", oracle._SO)
    with pytest.raises(RuntimeError, match="blsbn254_ctx_create"):
        M.load_library()


def test_library_exports_every_declared_symbol(M):
    lib = ctypes.CDLL(library_path_built())
    for s in declared_symbols():
        assert hasattr(lib, s), "missing export " + s


def test_no_cpu_fallback(M):
    """Without a GPU the engine must fail loudly, never compute on the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(M.Bn254Error) as e:
        M.Engine(0)
    assert e.value.code == -4
    lib = M.load_library()
    assert b"no CPU fallback" in lib.blsbn254_strerror(-4)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "bls-bn254_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp")):
                src = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "import oracle" not in src and "from oracle" not in src and "bn254_oracle" not in src, f


def test_error_class_mapping(M):
    assert M.InvalidScalarBytes.__mro__[1] is M.Bn254Error            # error.rs:4-10 order
    lib = M.load_library()
    assert [lib.blsbn254_strerror(i) for i in (1, 2, 3, 4)] == [b"invalid scalar bytes", b"invalid G1 bytes", b"invalid G2 bytes", b"invalid Gt bytes"]


def test_pack_messages(M):
    data, off = M.engine.pack_messages([b"", b"ab", b"cde"])
    assert data == b"abcde" and list(off) == [0, 0, 2, 5]


def test_header_is_valid_c_and_library_loads_from_a_c_program(tmp_path):
    """include/blsbn254.h compiled as strict C99 by a plain-C consumer that opens the shared library the way a cgo / Rust-FFI
    caller would (no HIP headers, no C++): every symbol it needs resolves, error strings match the reference's error names,
    and without a gfx950 device ctx_create fails loudly with BLSBN254_E_NO_DEVICE instead of falling back to a CPU path."""
    import subprocess
    exe = str(tmp_path / "consumer")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_c", "consumer.c"), "-o", exe, "-ldl"])
    lib = os.path.join(ROOT, "bls-bn254_amd", "libblsbn254_hip.so")
    out = subprocess.run([exe, lib], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert out.stdout.startswith("no device") or out.stdout.startswith("ctx ok")
