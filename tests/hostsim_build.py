"""The one compile recipe of the host-side test programs (tests/hostsim/*.cpp and bench_micro/lazy_tower_host.cpp): the device
headers compiled for the CPU, as a shared object for ctypes or as a stand-alone program.  A test tool; the product has no CPU
path.  Every test that needs such an artefact calls build(); nothing else under tests/ names the compiler."""
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM = os.path.join(ROOT, "tests", "hostsim")
CSRC = os.path.join(ROOT, "bls-bn254_amd", "csrc")

COMMON = ["-O1", "-std=c++17"]
CHECKED = ["-DBN_CHECK", "-pthread"]             # the recipe of every main file that FLAGS does not list
# per main file: what follows COMMON instead of CHECKED
FLAGS = {
    "hostsim.cpp": ["-DBN_CHECK", "-DBN_VERIFY_PARK_T", "-pthread"],
    "inflate_host.cpp": ["-DBN_CHECK"],
    "pair_product_host.cpp": ["-DBN_CHECK"],
    "seg_plan_host.cpp": ["-Wall", "-Werror"],
    "key_cache_host.cpp": ["-Wall", "-Wextra", "-Werror"],
    "rlc_plan_host.cpp": ["-Wall", "-Wextra", "-Werror"],
    "launch_forms_host.cpp": ["-Wall", "-Wextra", "-Werror"],
    "lazy_tower_host.cpp": [],
}
SANITIZED = ["-fsanitize=address,undefined", "-fno-sanitize-recover", "-g"]     # key_cache_host, rlc_plan_host and launch_forms_host only, run as programs of their own


def sources(main):
    """what an artefact is older than when it is stale: its main file, every device header, the headers beside the hostsim
    programs, and this recipe"""
    return [main] + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(SIM, "*.h")) + [os.path.abspath(__file__)]


def build(main, out, shared=True, extra=()):
    """Compile `main` into `out` (names under tests/hostsim/, or paths) -- a shared object, or a program when shared is false --
    unless `out` is already newer than all of sources(main); returns the path of `out`.  The compiler writes to a temporary name beside
    `out` that replaces it only when the compile succeeded, so a killed compile never leaves a fresh-looking artefact."""
    main, out = os.path.join(SIM, main), os.path.join(SIM, str(out))       # an absolute path stays what it is
    if os.path.exists(out) and all(os.path.getmtime(p) <= os.path.getmtime(out) for p in sources(main)):
        return out
    tmp = "%s.tmp%d.so" % (out, os.getpid())       # ends in .so whatever it is: git ignores it should a kill leave it behind
    flags = COMMON + FLAGS.get(os.path.basename(main), CHECKED) + (["-fPIC", "-shared"] if shared else []) + list(extra)
    try:
        subprocess.check_call(["g++"] + flags + ["-o", tmp, main])
        os.replace(tmp, out)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return out
