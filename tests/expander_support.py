"""The model the expander tests compare against: Keccak-f[1600] and the sponge in pure Python, the four digests / XOFs on top of
it, RFC 9380's expand_message for the five expander ids, and hash-to-field / hash-to-curve / sign composed from the pinned maps
of oracle/pyref/bn254.py.  Only the expander is new here.  tests/test_expander_model.py pins this file against hashlib, two
published Keccak-256 digests and the RFC's framing written out directly, before any other test relies on it.  CPU only."""
import hashlib

from oracle.pyref import bn254 as ref

XMD_SHA256, XMD_KECCAK256, XMD_SHA3_256, XOF_SHAKE128, XOF_SHAKE256 = range(5)
IDS = (XMD_SHA256, XMD_KECCAK256, XMD_SHA3_256, XOF_SHAKE128, XOF_SHAKE256)
M64 = (1 << 64) - 1


def _rol(v, n):
    return ((v << n) | (v >> (64 - n))) & M64


def keccak_f(a):
    """Keccak-f[1600] on 25 lanes a[x + 5 y] (FIPS 202 3.3); the offsets and constants are generated on the way"""
    a = list(a)
    reg = 1
    for _ in range(24):
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        for x in range(5):
            d = c[(x - 1) % 5] ^ _rol(c[(x + 1) % 5], 1)
            for y in range(0, 25, 5):
                a[x + y] ^= d
        x, y, cur = 1, 0, a[1]                      # rho and pi along the walk (x, y) -> (y, 2 x + 3 y)
        for t in range(24):
            x, y = y, (2 * x + 3 * y) % 5
            cur, a[x + 5 * y] = a[x + 5 * y], _rol(cur, ((t + 1) * (t + 2) // 2) % 64)
        for y in range(0, 25, 5):
            row = a[y:y + 5]
            for x in range(5):
                a[x + y] = row[x] ^ (~row[(x + 1) % 5] & M64 & row[(x + 2) % 5])
        for j in range(7):                          # iota: the LFSR of 3.2.5
            if reg & 1:
                a[0] ^= 1 << ((1 << j) - 1)
            reg = (reg << 1) ^ (0x171 if reg & 0x80 else 0)
    return a


def sponge(rate, domain, msg, n):
    """n bytes of Keccak[1600 - 8 rate](msg) under the domain byte: 0x01 Keccak, 0x06 SHA-3, 0x1F SHAKE"""
    m = bytearray(msg) + bytes([domain]) + bytes(-(len(msg) + 1) % rate)
    m[-1] |= 0x80
    a = [0] * 25
    for lo in range(0, len(m), rate):
        for k in range(rate // 8):
            a[k] ^= int.from_bytes(m[lo + 8 * k:lo + 8 * k + 8], "little")
        a = keccak_f(a)
    out = b""
    while len(out) < n:
        out += b"".join(w.to_bytes(8, "little") for w in a[:rate // 8])
        a = keccak_f(a)
    return out[:n]


def keccak256(m): return sponge(136, 0x01, m, 32)
def sha3_256(m): return sponge(136, 0x06, m, 32)
def shake128(m, n): return sponge(168, 0x1F, m, n)
def shake256(m, n): return sponge(136, 0x1F, m, n)


XMD_HASH = {XMD_SHA256: (lambda m: hashlib.sha256(m).digest(), 64), XMD_KECCAK256: (keccak256, 136), XMD_SHA3_256: (sha3_256, 136)}
XOF_HASH = {XOF_SHAKE128: shake128, XOF_SHAKE256: shake256}


def effective_dst(xid, dst):
    """RFC 9380 5.3.3: a tag longer than 255 bytes is replaced by 32 bytes of the expander's own hash"""
    if len(dst) <= 255:
        return dst
    if xid in XMD_HASH:
        return XMD_HASH[xid][0](b"H2C-OVERSIZE-DST-" + dst)
    return XOF_HASH[xid](b"H2C-OVERSIZE-DST-" + dst, 32)


def expand_message(xid, msg, dst, n):
    dst = effective_dst(xid, dst)
    dst_prime = dst + bytes([len(dst)])
    if xid in XOF_HASH:                             # RFC 9380 5.3.2
        return XOF_HASH[xid](msg + n.to_bytes(2, "big") + dst_prime, n)
    h, s_in_bytes = XMD_HASH[xid]                   # RFC 9380 5.3.1, b_in_bytes = 32
    ell = (n + 31) // 32
    assert ell <= 255
    b0 = h(bytes(s_in_bytes) + msg + n.to_bytes(2, "big") + b"\x00" + dst_prime)
    bi = h(b0 + b"\x01" + dst_prime)
    out = bi
    for i in range(2, ell + 1):
        bi = h(bytes(p ^ q for p, q in zip(b0, bi)) + bytes([i]) + dst_prime)
        out += bi
    return out[:n]


def hash_to_fp(xid, msg, dst, count):
    okm = expand_message(xid, msg, dst, 48 * count)
    return [int.from_bytes(okm[48 * i:48 * i + 48], "big") % ref.P for i in range(count)]


def hash_to_fp2(xid, msg, dst, count):
    u = hash_to_fp(xid, msg, dst, 2 * count)
    return [(u[2 * i], u[2 * i + 1]) for i in range(count)]


def hash_to_scalar(xid, msg, dst):
    return int.from_bytes(expand_message(xid, msg, dst, 48), "big") % ref.R


def hash_to_g1(xid, msg, dst):
    u0, u1 = hash_to_fp(xid, msg, dst, 2)
    return ref.g1_add(ref.svdw_g1(u0), ref.svdw_g1(u1))


def encode_to_g1(xid, msg, dst):
    return ref.svdw_g1(hash_to_fp(xid, msg, dst, 1)[0])


def hash_to_g2(xid, msg, dst):
    u0, u1 = hash_to_fp2(xid, msg, dst, 2)
    return ref.g2_clear_cofactor(ref.g2_add(ref.svdw_g2(u0), ref.svdw_g2(u1)))


def encode_to_g2(xid, msg, dst):
    return ref.g2_clear_cofactor(ref.svdw_g2(hash_to_fp2(xid, msg, dst, 1)[0]))


def sign(xid, sk, msg, dst):
    return ref.g1_mul(hash_to_g1(xid, msg, dst), sk % ref.R)


def boundary_messages(xid, dst):
    """messages whose absorbed length -- of b_0's input for the XMD forms, of msg' for the XOF forms -- is 0, 1, rate - 2 and
    rate - 1 modulo the rate (the pad is one 0x81-style byte, or spills into a block of its own), for an output of any length;
    then the empty message and one of 1000 bytes"""
    dl = len(effective_dst(xid, dst))
    rate = 168 if xid == XOF_SHAKE128 else 64 if xid == XMD_SHA256 else 136
    fixed = (2 + dl + 1) if xid in XOF_HASH else (rate + 2 + 1 + dl + 1)       # everything of the absorbed string but msg
    out = []
    for want in (0, 1, rate - 2, rate - 1):
        ln = (want - fixed) % rate
        out.append(bytes((7 * k + want) & 0xff for k in range(ln if ln else rate)))
    return out + [b"", bytes((k * k + 3) & 0xff for k in range(1000))]
