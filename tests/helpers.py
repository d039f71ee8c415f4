"""Small pure functions and constants that the host-side and the GPU tests share: byte encodings, bitmap rows, offsets of ragged
groups, the models of a few host-side rules.  One body per name: a variant that pads or types differently has a name of its own."""
import os
import re

import numpy as np

from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = synth.R
IDENT1 = bytes(32) + (1).to_bytes(32, "big")            # G1: x = 0, y = 1
IDENT2 = bytes(127) + b"\x01"                             # G2: x = 0, y = (c1 = 0, c0 = 1)


def b32(k):
    """32 bytes, big endian; int() so that numpy integers pass too"""
    return int(k).to_bytes(32, "big")


def row_of(sel, n):
    """the bitmap row of n bits, (n + 7) // 8 bytes, with the bits of sel set"""
    r = bytearray((n + 7) // 8)
    for i in sel:
        r[i >> 3] |= 1 << (i & 7)
    return bytes(r)


def bits_of(bm, n):
    """the first n bits of a bitmap as bools"""
    return [bool(bm[i >> 3] >> (i & 7) & 1) for i in range(n)]


def offsets_u64(sizes):
    """group offsets as the GPU calls take them"""
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


def bitmap(bools):
    """the bools as a bitmap with ONE SPARE BYTE behind the last used one (what the host-side programs are handed)"""
    out = bytearray((len(bools) + 7) // 8 + 1)
    for i, b in enumerate(bools):
        if b:
            out[i >> 3] |= 1 << (i & 7)
    return bytes(out)


def launches(n, cuts):
    """[lo, hi) pieces of 0 .. n cut at the given positions"""
    edges = [0] + [c for c in cuts if 0 < c < n] + [n]
    return [(a, b) for a, b in zip(edges, edges[1:]) if b > a]


def u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def model_candidate(sig, p):
    """decodes (both coordinates below p), not the identity (x == 0 reads as it), on y^2 = x^3 + 3"""
    x, y = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
    return x < p and y < p and x != 0 and (y * y - x * x * x - 3) % p == 0


def poly_eval(coeffs, x):
    """Horner in Fr"""
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def glv_lambda():
    src = open(os.path.join(ROOT, "bls-bn254_amd", "csrc", "bn254_consts.h")).read()
    words = re.search(r"GLV_LAMBDA\[4\]\s*=\s*\{([^}]*)\}", src).group(1).split(",")
    return sum(int(w.strip().rstrip("uUlL"), 16) << (64 * i) for i, w in enumerate(words))


# coefficients where the 9 x 29-bit limb form and its carries can go wrong: the ends of the range, limb boundaries, long carry runs
EDGE_COEFFS = (0, 1, synth.P - 1, 2, synth.P - 2, (synth.P + 1) // 2, (synth.P - 1) // 2, 1 << 29, (1 << 29) - 1, 1 << 58, 1 << 232, (1 << 232) - 1,
               1 << 253, (1 << 253) - 1, synth.P // 3, 3)


def rand_coeffs(seed, n, per):
    """n elements of `per` canonical 32-byte big-endian coefficients (top byte < 0x30 keeps every value below p); the first
    coefficients carry EDGE_COEFFS."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=(n * per, 32), dtype=np.uint8)
    a[:, 0] %= 0x30
    for k, v in enumerate(EDGE_COEFFS[:min(len(EDGE_COEFFS), n * per)]):
        a[k] = np.frombuffer(v.to_bytes(32, "big"), dtype=np.uint8)
    return a.tobytes()


def offsets_u32(sizes):
    """group offsets as the host-side lane functions take them"""
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
