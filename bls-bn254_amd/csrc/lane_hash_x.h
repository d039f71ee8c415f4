// lane_hash_x.h -- what ONE lane does for ONE message in the hashing kernels that take the expander as an argument
// (k_hash_keccak.hip): the lane functions of lane_ops.h / keygen.h with expand_message(xid, ...) (keccak.h) in the place of
// expand_message_xmd.  The maps, the field code and the reductions are the ones those functions call.  Compiled for the host by
// tests/hostsim/keccak_host.cpp (-DBN_CHECK: the interval checks over the new path into fp_from_okm); not a CPU fallback.
#pragma once
#include "lane_ops.h"
#include "fr29.h"
#include "keccak.h"

namespace bn {

BN_FUNC G1A lane_hash_to_g1_x(uint32_t xid, const uint8_t* msg, size_t msg_len, const uint8_t* dst, uint32_t dst_len) {       // g1.rs:910-919
  uint8_t okm[96];
  expand_message(xid, okm, 96, msg, msg_len, dst, dst_len);
  return hash_to_g1_from_fields(fp_from_okm(okm), fp_from_okm(okm + 48));
}
BN_FUNC G1P lane_hash_to_g1_proj_x(uint32_t xid, const uint8_t* msg, size_t msg_len, const uint8_t* dst, uint32_t dst_len) {
  uint8_t okm[96];
  expand_message(xid, okm, 96, msg, msg_len, dst, dst_len);
  return hash_to_g1_from_fields_proj(fp_from_okm(okm), fp_from_okm(okm + 48));
}
BN_FUNC G1A lane_encode_to_g1_x(uint32_t xid, const uint8_t* msg, size_t msg_len, const uint8_t* dst, uint32_t dst_len) {     // g1.rs:922-928
  uint8_t okm[48];
  expand_message(xid, okm, 48, msg, msg_len, dst, dst_len);
  return svdw_g1(fp_from_okm(okm));
}
BN_FUNC G2A lane_hash_to_g2_x(uint32_t xid, const uint8_t* msg, size_t msg_len, const uint8_t* dst, uint32_t dst_len, bool ro) {  // g2.rs:919-936
  uint8_t okm[192];
  expand_message(xid, okm, ro ? 192 : 96, msg, msg_len, dst, dst_len);
  Fp2 u0 = {fp_from_okm(okm), fp_from_okm(okm + 48)};
  G2P q = proj_from_affine(svdw_g2(u0));
  if (ro) {
    Fp2 u1 = {fp_from_okm(okm + 96), fp_from_okm(okm + 144)};
    q = proj_add(q, proj_from_affine(svdw_g2(u1)));
  }
  return g2_to_affine(g2_clear_cofactor(q));
}
BN_FUNC Fr lane_hash_to_scalar_x(uint32_t xid, const uint8_t* msg, size_t msg_len, const uint8_t* dst, uint32_t dst_len) {    // scalar.rs:554-563
  uint8_t okm[48];
  expand_message(xid, okm, 48, msg, msg_len, dst, dst_len);
  return fr_from_okm(okm);
}

}  // namespace bn
