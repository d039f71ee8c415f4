"""Keccak-f[1600] of the all-zero state: the constant that expand_message_xmd_keccak (keccak.h, keccak_init_zpad) starts b_0
from.  Z_pad of the XMD forms over Keccak-256 and SHA3-256 is s_in_bytes = 136 zero bytes, exactly one block at their rate, so
the state after absorbing it is the permutation of zero whatever follows.  Computed here from FIPS 202 alone: the rotation
offsets from the (t + 1)(t + 2) / 2 walk of section 3.2.2, the round constants from the LFSR of section 3.2.5; no hashlib.
tests/test_keccak_host.py imports zero_state() and compares it with the header (and recomputes it with the tests' own model).
Usage: python scripts/keccak_zero_block_state.py"""

M64 = (1 << 64) - 1


def rotation_offsets():
    """r[x + 5 y] of FIPS 202 3.2.2 (rho)"""
    r = [0] * 25
    x, y = 1, 0
    for t in range(24):
        r[x + 5 * y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return r


def round_constants():
    """RC[0 .. 24) of FIPS 202 3.2.5 (iota): bit 2^j - 1 of RC[i] is rc(j + 7 i)"""
    out, reg = [], 1
    for _ in range(24):
        rc = 0
        for j in range(7):
            if reg & 1:
                rc |= 1 << ((1 << j) - 1)
            reg <<= 1
            if reg & 0x100:
                reg ^= 0x171
        out.append(rc)
    return out


RHO = rotation_offsets()
RC = round_constants()


def rol(v, n):
    return ((v << n) | (v >> (64 - n))) & M64 if n else v


def keccak_f(a):
    """the permutation on 25 lanes, a[x + 5 y]"""
    a = list(a)
    for rc in RC:
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x + 4) % 5] ^ rol(c[(x + 1) % 5], 1) for x in range(5)]
        a = [a[i] ^ d[i % 5] for i in range(25)]
        b = [0] * 25
        for x in range(5):
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = rol(a[x + 5 * y], RHO[x + 5 * y])
        a = [b[i] ^ (~b[(i % 5 + 1) % 5 + 5 * (i // 5)] & M64 & b[(i % 5 + 2) % 5 + 5 * (i // 5)]) for i in range(25)]
        a[0] ^= rc
    return a


def zero_state():
    return keccak_f([0] * 25)


if __name__ == "__main__":
    print("RHO:", ", ".join(str(x) for x in RHO))
    print("RC:", ", ".join("0x%016x" % x for x in RC))
    z = zero_state()
    for k in range(0, 25, 5):
        print(", ".join("0x%016xull" % x for x in z[k:k + 5]) + ",")
