// keyset_rlc.h -- what ONE lane does in the key-set FastAggregateVerify by random linear combination per message
// (k_keyset_rlc.hip, host_keyset_rlc.hip).  For groups g that share a message m, with key sums S_g and
// signatures sig_g,
//     prod_g [ e(sig_g, -G2gen) e(H(m), S_g) ]^(r_g)  =  e(sum_g r_g sig_g, -G2gen) e(H(m), sum_g r_g S_g)
// so one pairing equation decides a whole chunk of groups.  The weighted sum on the G2 side needs every S_g in the r-torsion:
// a group is ELIGIBLE only when every key it adds has the KeyValidate bit (a sum of r-torsion points is in the r-torsion), and
// everything else keeps the exact path.
//   ksr_row_valid       no selected, non-skipped key of a row lacks the KeyValidate bit (registry words, or a committee's)
//   ksr_sig_ok          the signature decodes, is on the curve and is not the identity
//   ksr_is_identity     Z = 0 of a stored homogeneous G2 point
//   ksr_weight          r_g: the first 8 bytes, big-endian, of SHA-256(seed || "KSRLC" || g as 8 bytes LE || sig_g); 0 becomes 1
//   ksr_mul_u64         [r] P by branch-free double-and-add over the complete formulas, G1 and G2
//   ksr_chunk_state     what becomes of a chunk once its sums are known
// keyset_rlc_plan.h is the plain C++ of the host side.  tests/hostsim/keyset_rlc_host.cpp compiles both for the host with
// -DBN_CHECK.  The lane functions are not a CPU fallback: nothing in the product's host path calls them.
#pragma once
#include "keyset.h"
#include "keyset_rlc_plan.h"

namespace bn {

BN_INL bool ksr_row_valid(const uint8_t* row, uint32_t n_keys, const uint32_t* skip, const uint32_t* valid) {
  const uint32_t W = ks_words(n_keys), rb = ks_row_bytes(n_keys);
  uint32_t miss = 0;
#pragma unroll 4
  for (uint32_t w = 0; w < W; ++w) miss |= ks_row_word(row, rb, w) & ks_tail_mask(n_keys, w) & ~skip[w] & ~valid[w];
  return miss == 0;
}
BN_FUNC bool ksr_sig_ok(const uint8_t* sig, G1A& p) {
  bool ok;
  p = g1_decode(sig, ok);
  return ok & !p.inf & g1_on_curve(p);
}
// ws: a point stored by ks_store_point (canonical limbs)
BN_INL bool ksr_is_identity(const int32_t* ws, size_t stride) {
  int32_t any = 0;
  for (int k = 4 * NL; k < 6 * NL; ++k) any |= ws[(size_t)k * stride];
  return any == 0;
}
BN_INL bool ksr_eligible(bool row_ok, bool row_valid, bool sig_ok, bool sum_identity) { return row_ok & row_valid & sig_ok & !sum_identity; }

BN_INL uint64_t ksr_weight_of_digest(const uint8_t* dg) {
  uint64_t r = 0;
  for (int k = 0; k < 8; ++k) r = (r << 8) | dg[k];
  return r ? r : 1;
}
BN_FUNC uint64_t ksr_weight(const uint8_t* seed, uint64_t g, const uint8_t* sig) {
  const uint8_t tag[5] = {'K', 'S', 'R', 'L', 'C'};
  Sha256 s; sha256_init(s);
  sha256_update(s, seed, 32);
  sha256_update(s, tag, 5);
  for (int k = 0; k < 8; ++k) sha256_byte(s, (uint8_t)(g >> (8 * k)));
  sha256_update(s, sig, 64);
  uint8_t dg[32]; sha256_final(s, dg);
  return ksr_weight_of_digest(dg);
}

// 64 doublings and 64 additions whatever the bits: the lanes of a wave carry different weights
template <class F> BN_FUNC Proj<F> ksr_mul_u64(const Proj<F>& p, uint64_t k) {
  BN_CTX;
  Proj<F> acc = proj_identity<F>();
#pragma unroll 1
  for (int i = 63; i >= 0; --i) {
    acc = proj_dbl(acc);
    const Proj<F> s = proj_add(acc, p);
    acc = proj_select((k >> i) & 1, s, acc);
  }
  return acc;
}

// fewer than two eligible members: nothing to be gained; a sum that is the identity cannot go through the verify pipeline
BN_INL uint8_t ksr_chunk_state(uint32_t eligible, bool sa_identity, bool sb_identity) {
  return eligible < 2 ? KSR_DIRECT : (sa_identity | sb_identity) ? KSR_DEGENERATE : KSR_CHECK;
}

}  // namespace bn
