"""The SHA-256 state after one block of 64 zero bytes: the constant that expand_message_xmd (sha256.h, SHA256_ZPAD_STATE)
starts b_0 from, since Z_pad is always that block.  Computed here from FIPS 180-4 alone: the round constants are the first 32
fractional bits of the cube roots of the first 64 primes, the initial state those of the square roots of the first 8, both
derived with integer arithmetic; no hashlib.  tests/test_op_trim.py imports zero_block_state() and compares it with the header.
Usage: python scripts/sha256_zero_block_state.py"""

M32 = 0xFFFFFFFF


def primes(n):
    out, c = [], 2
    while len(out) < n:
        if all(c % q for q in out if q * q <= c):
            out.append(c)
        c += 1
    return out


def iroot(x, k):
    lo, hi = 0, 1 << (x.bit_length() // k + 2)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if mid ** k <= x:
            lo = mid
        else:
            hi = mid - 1
    return lo


def frac32(p, k):          # first 32 fractional bits of p^(1/k)
    return iroot(p << (32 * k), k) & M32


K = [frac32(p, 3) for p in primes(64)]
IV = [frac32(p, 2) for p in primes(8)]


def ror(x, n):
    return ((x >> n) | (x << (32 - n))) & M32


def compress(h, block):
    """One FIPS 180-4 compression: h = 8 words, block = 64 bytes."""
    w = [int.from_bytes(block[4 * i:4 * i + 4], "big") for i in range(16)]
    for i in range(16, 64):
        s0 = ror(w[i - 15], 7) ^ ror(w[i - 15], 18) ^ (w[i - 15] >> 3)
        s1 = ror(w[i - 2], 17) ^ ror(w[i - 2], 19) ^ (w[i - 2] >> 10)
        w.append((w[i - 16] + s0 + w[i - 7] + s1) & M32)
    a, b, c, d, e, f, g, hh = h
    for i in range(64):
        t1 = (hh + (ror(e, 6) ^ ror(e, 11) ^ ror(e, 25)) + ((e & f) ^ (~e & M32 & g)) + K[i] + w[i]) & M32
        t2 = ((ror(a, 2) ^ ror(a, 13) ^ ror(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & M32
        hh, g, f, e, d, c, b, a = g, f, e, (d + t1) & M32, c, b, a, (t1 + t2) & M32
    return [(x + y) & M32 for x, y in zip(h, (a, b, c, d, e, f, g, hh))]


def sha256(msg):
    """The whole hash from compress(), to check compress() against known digests."""
    m = msg + b"\x80" + bytes((55 - len(msg)) % 64) + (8 * len(msg)).to_bytes(8, "big")
    h = list(IV)
    for i in range(0, len(m), 64):
        h = compress(h, m[i:i + 64])
    return b"".join(x.to_bytes(4, "big") for x in h)


def zero_block_state():
    return compress(list(IV), bytes(64))


if __name__ == "__main__":
    print(", ".join("0x%08x" % x for x in zero_block_state()))
