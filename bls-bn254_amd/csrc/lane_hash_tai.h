// lane_hash_tai.h -- what ONE lane does for ONE message under the try-and-increment map to G1 (blsbn254_set_g1_map; the map of
// the EVM's BN254 BLS contracts): the start value x0 from the message or from its plain digest, one candidate's
// right-hand side, the step to the next candidate, the sequential search, and the point behind the x that won.  The kernels of
// k_hash_tai.hip are built from these; their pooled search tests the same candidates with the same functions, dealt over the
// lanes of a wave.  Compiled for the host by tests/hostsim/g1_map_host.cpp (-DBN_CHECK: the interval checks over the whole
// path); not a CPU fallback.
//   x0:     TAI_DIGEST: the message bytes as ONE big-endian integer mod p (32 bytes: uint256(h) % p; any other length the same
//           way, 32 bytes at a time -- a total function, no security claim).  TAI_HASH: the 32-byte plain digest of the message
//           under the hash of the context's expander (no tag, no padding block), reduced the same way.
//   search: k = 0, 1, 2, ...: x = x0 + k mod p, beta = x^3 + 3; the first x whose beta is a square wins.  The test is the Jacobi
//           symbol (fp_is_square), no power.  beta == 0 cannot happen: (x, 0) would be a point of order 2 on a curve of prime
//           order, so there is no code path for it (fp_is_square counts 0 as a square, and nothing depends on that).
//   point:  (x, beta^((p+1)/4)) = (x, beta * beta^((p-3)/4)), the fixed chain of fp29.h, ONCE per message.  Exactly that root:
//           no sign rule, no negation.
// Every loop is bounded: the search stops after TAI_CAP candidates and the lane then yields (0, 0), which is not on the curve.
// No known input comes near the cap (a run of c non-residues has probability 2^-c); it is there so that a wrong square test
// cannot spin a wave.  tests/hostsim builds a second copy with -DTAI_CAP=4 to reach it.
#pragma once
#include "lane_ops.h"
#include "keccak.h"

#ifndef TAI_CAP
#define TAI_CAP 65536
#endif

namespace bn {

enum : uint32_t { G1MAP_SVDW = 0, G1MAP_TAI_DIGEST = 1, G1MAP_TAI_HASH = 2, G1MAP_COUNT = 3 };

// 32 bytes: the first 32 of H(msg), H the plain hash behind the expander xid (keccak.h EXPAND_*)
BN_FUNC void tai_plain_digest(uint32_t xid, uint8_t out[32], const uint8_t* msg, size_t msg_len) {
  if (xid == EXPAND_XMD_SHA256) {
    Sha256 s;
    sha256_init(s); sha256_update(s, msg, msg_len); sha256_final(s, out);
    return;
  }
  const uint32_t rate = xid == EXPAND_XOF_SHAKE128 ? KECCAK_RATE_128 : KECCAK_RATE_256;
  const uint8_t domain = xid == EXPAND_XMD_KECCAK256 ? KECCAK_DOMAIN_KECCAK : xid == EXPAND_XMD_SHA3_256 ? KECCAK_DOMAIN_SHA3 : KECCAK_DOMAIN_SHAKE;
  keccak_hash(out, 32, msg, msg_len, rate, domain);
}

// len bytes as one big-endian integer mod p (Montgomery form).  Up to 32 bytes: one decode, whose product with R^2 reduces any
// 256-bit value.  Longer: Horner over 32-byte pieces, the leading piece the short one, with 2^256 = (2^128)^2 as the multiplier.
BN_FUNC Fp tai_from_bytes(const uint8_t* b, size_t len) {
  BN_CTX;
  uint8_t piece[32];
  bool ok;
  const size_t head = len % 32 ? len % 32 : (len ? 32 : 0);
  for (size_t j = 0; j < 32; ++j) piece[j] = j < 32 - head ? 0 : b[j - (32 - head)];
  Fp x = fp_from_be(piece, ok);
  if (len <= 32) return x;
  for (size_t j = 0; j < 32; ++j) piece[j] = j == 15 ? 1 : 0;
  const Fp two128 = fp_from_be(piece, ok);
  const Fp two256 = fp_sqr(two128);
  for (size_t at = head; at < len; at += 32) {
    for (size_t j = 0; j < 32; ++j) piece[j] = b[at + j];
    x = fp_norm(fp_add(fp_mul(x, two256), fp_from_be(piece, ok)));
  }
  return x;
}

BN_FUNC Fp tai_x0(uint32_t map, uint32_t xid, const uint8_t* msg, size_t msg_len) {
  if (map == G1MAP_TAI_DIGEST) return tai_from_bytes(msg, msg_len);
  uint8_t d[32];
  tai_plain_digest(xid, d, msg, msg_len);
  return tai_from_bytes(d, 32);
}

// beta = x^3 + 3
BN_FUNC Fp tai_rhs(const Fp& x) { return fp_norm(fp_add(fp_mul(fp_sqr(x), x), fp_const(bnc::THREE))); }
// x + k for a small k (< 2^29), through one product that brings the sum back into the range every product leaves: a search may
// take TAI_CAP steps, and lazily added ones would outgrow the limbs after 160
BN_FUNC Fp tai_offset(const Fp& x, uint32_t k) {
  Fp kp = fp_zero();
  kp.l[0] = (int32_t)k;
  BN_TRK(set_trk(kp, 0, 1, 0, 0, 1e-60);)
  return fp_norm(fp_add(x, fp_to_mont(kp)));
}

// The contract's loop, one candidate after the other.  true: x is the winner and k its distance from x0; false: TAI_CAP
// candidates were non-residues
BN_FUNC bool tai_search(Fp& x, uint32_t& k) {
  BN_CTX;
  const Fp x0 = x;
  for (k = 0; k < (uint32_t)TAI_CAP; ++k) {
    x = tai_offset(x0, k);
    if (fp_is_square(tai_rhs(x))) return true;
  }
  return false;
}

// the point of the winner, or (0, 0) for a search that hit the cap
BN_FUNC G1A tai_point(const Fp& x, bool found) {
  BN_CTX;
  const Fp beta = tai_rhs(x);
  const Fp y = fp_mul(beta, fp_pow_pm3_4(beta));
  G1A h;
  h.x = fp_select(found, x, fp_zero());
  h.y = fp_select(found, y, fp_zero());
  h.inf = false;
  return h;
}

BN_FUNC G1A lane_hash_to_g1_tai(uint32_t map, uint32_t xid, const uint8_t* msg, size_t msg_len) {
  Fp x = tai_x0(map, xid, msg, msg_len);
  uint32_t k;
  const bool found = tai_search(x, k);
  return tai_point(x, found);
}

}  // namespace bn
