// keccak.h -- FIPS 202 Keccak-f[1600], a byte-wise sponge, and the message expanders of RFC 9380 built on it, one instance per
// lane: expand_message_xmd (5.3.1) over Keccak-256 / SHA3-256 and expand_message_xof (5.3.2) over SHAKE-128 / SHAKE-256.  With
// sha256.h these are the instantiations of X: ExpandMsg that Fp::hash<X> / Fp::encode<X> (fp.rs:433-458), Fp2::hash<X>
// (fp2.rs:463-487), G1Projective::hash<X> / encode<X> (g1.rs:910-928), G2Projective::hash<X> / encode<X> (g2.rs:919-936) and
// Scalar::hash<X> (scalar.rs:554-563) are generic over: ExpandMsgXmd<Sha256 | Keccak256 | Sha3_256>, ExpandMsgXof<Shake128 | Shake256>.
// 64-bit lanes as register pairs: XOR / AND-NOT are 32-bit VALU work, every rotate is a pair of 32-bit funnel shifts.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "sha256.h"

namespace bn {

// the expander of a launch (include/blsbn254.h BLSBN254_EXPAND_*): uniform over the lanes
enum : uint32_t { EXPAND_XMD_SHA256 = 0, EXPAND_XMD_KECCAK256 = 1, EXPAND_XMD_SHA3_256 = 2, EXPAND_XOF_SHAKE128 = 3, EXPAND_XOF_SHAKE256 = 4, EXPAND_COUNT = 5 };
enum : uint8_t { KECCAK_DOMAIN_KECCAK = 0x01, KECCAK_DOMAIN_SHA3 = 0x06, KECCAK_DOMAIN_SHAKE = 0x1F };
enum : uint32_t { KECCAK_RATE_256 = 136, KECCAK_RATE_128 = 168 };      // bytes per block at capacity 512 / 256

struct Keccak {
  uint64_t a[25];      // the state, lane x + 5 y: indexed by a run-time value while absorbing, so it lives in scratch
  uint64_t cur;        // absorbing: the lane being assembled; squeezing: what is left of the lane being handed out
  uint32_t fill;       // bytes taken into (absorbing) or out of (squeezing) the current block
  uint32_t rate;
};

// rotate left by 0 <= n < 64.  On the device as two v_alignbit_b32 over the swapped or unswapped halves; n is a constant at every call site
BN_INL uint64_t rotl64(uint64_t v, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  if (n & 32) { const uint32_t t = lo; lo = hi; hi = t; }
  n &= 31;
  if (n) {
    const uint32_t l2 = __builtin_amdgcn_alignbit(lo, hi, 32 - n), h2 = __builtin_amdgcn_alignbit(hi, lo, 32 - n);
    lo = l2; hi = h2;
  }
  return ((uint64_t)hi << 32) | lo;
#else
  return n ? (v << n) | (v >> (64 - n)) : v;
#endif
}

// A real function on the device, as sha256_compress is and for its reason: the byte-wise sponge below has a permutation behind
// every "block full" test and every squeeze, and a round is ~300 instructions.  The rounds stay a loop (24 x one body, the round
// constant a uniform load): the function is about one round long and the state never leaves the registers inside it.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BN_KECCAK_INLINE)
#define BN_KECCAK_FUNC BN_HD __attribute__((noinline))
#else
#define BN_KECCAK_FUNC BN_FUNC
#endif
BN_KECCAK_FUNC void keccak_f(uint64_t* st) {
  // FIPS 202 3.2.5 (scripts/keccak_zero_block_state.py derives them from the LFSR)
  const uint64_t RC[24] = {
      0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull, 0x0000000080000001ull,
      0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
      0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
      0x000000000000800aull, 0x800000008000000aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
  // rho offsets of lane x + 5 y (3.2.2; the same script)
  constexpr int RHO[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
  uint64_t a[25];
  BN_UNROLL for (int i = 0; i < 25; ++i) a[i] = st[i];
#pragma unroll 1
  for (int round = 0; round < 24; ++round) {
    uint64_t c[5], b[25];
    BN_UNROLL for (int x = 0; x < 5; ++x) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];                  // theta
    BN_UNROLL for (int x = 0; x < 5; ++x) {
      const uint64_t d = c[(x + 4) % 5] ^ rotl64(c[(x + 1) % 5], 1);
      BN_UNROLL for (int y = 0; y < 5; ++y) a[x + 5 * y] ^= d;
    }
    BN_UNROLL for (int x = 0; x < 5; ++x)                                                                             // rho, pi
      BN_UNROLL for (int y = 0; y < 5; ++y) b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl64(a[x + 5 * y], RHO[x + 5 * y]);
    BN_UNROLL for (int y = 0; y < 5; ++y)                                                                             // chi
      BN_UNROLL for (int x = 0; x < 5; ++x) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
    a[0] ^= RC[round];                                                                                                // iota
  }
  BN_UNROLL for (int i = 0; i < 25; ++i) st[i] = a[i];
}

BN_FUNC void keccak_init(Keccak& s, uint32_t rate) {
  for (int i = 0; i < 25; ++i) s.a[i] = 0;
  s.cur = 0; s.fill = 0; s.rate = rate;
}
// Keccak-f(0): the state after ONE block of zeros at any rate (scripts/keccak_zero_block_state.py derives it from FIPS 202;
// tests/test_keccak_host.py recomputes it).  Z_pad of expand_message_xmd is s_in_bytes = 136 zero bytes, the whole first block
// of Keccak-256 / SHA3-256: b_0 starts here, one permutation of its hash saved.
BN_FUNC void keccak_init_zpad(Keccak& s) {
  const uint64_t Z[25] = {
      0xf1258f7940e1dde7ull, 0x84d5ccf933c0478aull, 0xd598261ea65aa9eeull, 0xbd1547306f80494dull, 0x8b284e056253d057ull,
      0xff97a42d7f8e6fd4ull, 0x90fee5a0a44647c4ull, 0x8c5bda0cd6192e76ull, 0xad30a6f71b19059cull, 0x30935ab7d08ffc64ull,
      0xeb5aa93f2317d635ull, 0xa9a6e6260d712103ull, 0x81a57c16dbcf555full, 0x43b831cd0347c826ull, 0x01f22f1a11a5569full,
      0x05e5635a21d9ae61ull, 0x64befef28cc970f2ull, 0x613670957bc46611ull, 0xb87c5a554fd00ecbull, 0x8c3ee88a1ccf32c8ull,
      0x940c7922ae3a2614ull, 0x1841f924a2c509e4ull, 0x16f53526e70465c2ull, 0x75f644e97f30a13bull, 0xeaf1ff7b5ceca249ull};
  for (int i = 0; i < 25; ++i) s.a[i] = Z[i];
  s.cur = 0; s.fill = 0; s.rate = KECCAK_RATE_256;
}
// One byte: assembled in a register (little-endian within the lane), folded into the state once per completed lane -- a
// read-modify-write of the run-time-indexed state per byte would be a scratch round trip per byte.  Both rates are whole lanes.
BN_FUNC void keccak_byte(Keccak& s, uint8_t b) {
  s.cur |= (uint64_t)b << (8 * (s.fill & 7));
  ++s.fill;
  if ((s.fill & 7) == 0) {
    s.a[(s.fill >> 3) - 1] ^= s.cur;
    s.cur = 0;
    if (s.fill == s.rate) { keccak_f(s.a); s.fill = 0; }
  }
}
BN_FUNC void keccak_update(Keccak& s, const uint8_t* p, size_t n) { for (size_t i = 0; i < n; ++i) keccak_byte(s, p[i]); }
// pad10*1 behind the domain byte (0x01 Keccak, 0x06 SHA-3, 0x1F SHAKE), then the sponge turns to squeezing: fill < rate here, so
// the lane in `cur` is incomplete, and when fill == rate - 1 both pad ends meet in one byte (0x81 / 0x86 / 0x9F)
BN_FUNC void keccak_finish(Keccak& s, uint8_t domain) {
  s.cur |= (uint64_t)domain << (8 * (s.fill & 7));
  s.a[s.fill >> 3] ^= s.cur;
  s.a[(s.rate >> 3) - 1] ^= 0x8000000000000000ull;
  keccak_f(s.a);
  s.cur = 0; s.fill = 0;
}
// n more bytes of output; a lane is read once and handed out byte by byte, and a squeeze may cross a rate boundary
BN_FUNC void keccak_squeeze(Keccak& s, uint8_t* out, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    if ((s.fill & 7) == 0) {
      if (s.fill == s.rate) { keccak_f(s.a); s.fill = 0; }
      s.cur = s.a[s.fill >> 3];
    }
    out[i] = (uint8_t)s.cur;
    s.cur >>= 8; ++s.fill;
  }
}
// the whole hash in one call (host side: the oversize-DST rule; tests)
BN_FUNC void keccak_hash(uint8_t* out, size_t n, const uint8_t* msg, size_t msg_len, uint32_t rate, uint8_t domain) {
  Keccak s;
  keccak_init(s, rate);
  keccak_update(s, msg, msg_len);
  keccak_finish(s, domain);
  keccak_squeeze(s, out, n);
}

// out[0..n) = expand_message_xmd(msg, dst, n) over Keccak-256 (domain 0x01) or SHA3-256 (0x06): RFC 9380 5.3.1 with
// b_in_bytes = 32, s_in_bytes = 136; n <= 192 here (ell <= 6), dst_len <= 255 (a longer DST is pre-hashed on the host, 5.3.3)
BN_FUNC void expand_message_xmd_keccak(uint8_t* out, uint32_t n, const uint8_t* msg, size_t msg_len, const uint8_t* dst, uint32_t dst_len,
                                       uint8_t domain) {
  uint8_t b0[32], bi[32];
  Keccak s;
  keccak_init_zpad(s);                                            // Z_pad: the state after its block is a constant
  keccak_update(s, msg, msg_len);
  keccak_byte(s, (uint8_t)(n >> 8)); keccak_byte(s, (uint8_t)n); keccak_byte(s, 0);
  keccak_update(s, dst, dst_len); keccak_byte(s, (uint8_t)dst_len);
  keccak_finish(s, domain); keccak_squeeze(s, b0, 32);
  keccak_init(s, KECCAK_RATE_256);
  keccak_update(s, b0, 32); keccak_byte(s, 1);
  keccak_update(s, dst, dst_len); keccak_byte(s, (uint8_t)dst_len);
  keccak_finish(s, domain); keccak_squeeze(s, bi, 32);
  uint32_t ell = (n + 31) / 32, done = 0;
  for (uint32_t i = 1; i <= ell; ++i) {
    for (uint32_t k = 0; k < 32 && done < n; ++k) out[done++] = bi[k];
    if (i == ell) break;
    keccak_init(s, KECCAK_RATE_256);
    for (int k = 0; k < 32; ++k) keccak_byte(s, b0[k] ^ bi[k]);
    keccak_byte(s, (uint8_t)(i + 1));
    keccak_update(s, dst, dst_len); keccak_byte(s, (uint8_t)dst_len);
    keccak_finish(s, domain); keccak_squeeze(s, bi, 32);
  }
}
// out[0..n) = expand_message_xof(msg, dst, n) = H(msg || I2OSP(n, 2) || dst || I2OSP(dst_len, 1), n) over SHAKE-128 (rate 168) or
// SHAKE-256 (rate 136): RFC 9380 5.3.2; dst_len <= 255 as above
BN_FUNC void expand_message_xof(uint8_t* out, uint32_t n, const uint8_t* msg, size_t msg_len, const uint8_t* dst, uint32_t dst_len, uint32_t rate) {
  Keccak s;
  keccak_init(s, rate);
  keccak_update(s, msg, msg_len);
  keccak_byte(s, (uint8_t)(n >> 8)); keccak_byte(s, (uint8_t)n);
  keccak_update(s, dst, dst_len); keccak_byte(s, (uint8_t)dst_len);
  keccak_finish(s, KECCAK_DOMAIN_SHAKE);
  keccak_squeeze(s, out, n);
}
// THE dispatcher: xid is one of EXPAND_* and uniform over a launch, so the branches do not diverge
BN_FUNC void expand_message(uint32_t xid, uint8_t* out, uint32_t n, const uint8_t* msg, size_t msg_len, const uint8_t* dst, uint32_t dst_len) {
  if (xid == EXPAND_XMD_SHA256) expand_message_xmd(out, n, msg, msg_len, dst, dst_len);
  else if (xid == EXPAND_XMD_KECCAK256) expand_message_xmd_keccak(out, n, msg, msg_len, dst, dst_len, KECCAK_DOMAIN_KECCAK);
  else if (xid == EXPAND_XMD_SHA3_256) expand_message_xmd_keccak(out, n, msg, msg_len, dst, dst_len, KECCAK_DOMAIN_SHA3);
  else expand_message_xof(out, n, msg, msg_len, dst, dst_len, xid == EXPAND_XOF_SHAKE128 ? KECCAK_RATE_128 : KECCAK_RATE_256);
}
// RFC 9380 5.3.3 under expander xid: the 32 bytes that stand for a DST longer than 255 bytes -- H("H2C-OVERSIZE-DST-" || dst) for
// the XMD forms, H(..., ceil(2 k / 8)) with k = 128 for the XOF forms.  Host side (stage_dst); tests.
BN_FUNC void oversize_dst(uint32_t xid, uint8_t out[32], const uint8_t* dst, size_t dst_len) {
  const uint8_t tag[17] = {'H', '2', 'C', '-', 'O', 'V', 'E', 'R', 'S', 'I', 'Z', 'E', '-', 'D', 'S', 'T', '-'};
  if (xid == EXPAND_XMD_SHA256) {
    Sha256 s; sha256_init(s);
    sha256_update(s, tag, 17); sha256_update(s, dst, dst_len); sha256_final(s, out);
    return;
  }
  Keccak s;
  keccak_init(s, xid == EXPAND_XOF_SHAKE128 ? KECCAK_RATE_128 : KECCAK_RATE_256);
  keccak_update(s, tag, 17); keccak_update(s, dst, dst_len);
  keccak_finish(s, xid == EXPAND_XMD_KECCAK256 ? KECCAK_DOMAIN_KECCAK : xid == EXPAND_XMD_SHA3_256 ? KECCAK_DOMAIN_SHA3 : KECCAK_DOMAIN_SHAKE);
  keccak_squeeze(s, out, 32);
}

}  // namespace bn
