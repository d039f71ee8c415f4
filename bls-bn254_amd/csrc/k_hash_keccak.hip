// k_hash_keccak.hip -- the four hashing kernels with the message expander as a run-time argument (keccak.h: XMD over Keccak-256 /
// SHA3-256, XOF over SHAKE-128 / SHAKE-256): the siblings of k_hash_to_g1 (k_hash_g1.hip), k_hash_to_g2 (k_misc.hip), k_sign
// (k_sign.hip) and k_hash_to_scalar (k_keygen.hip), which stay XMD-SHA-256 and untouched.  The host launches these for every
// expander but the default (host_common.h launch_hash_to_g1 and its siblings).  One body per kernel: xid is uniform over a launch.
// Own translation unit under k_hash_g1.hip's policy (-DBN_FORCE_INLINE, two waves per SIMD for the G1 and scalar kernels); the
// permutation itself is a real function (keccak.h).  Same arguments, same workspace layouts and modes as the SHA-256 kernels.
#include "lane_hash_x.h"
#include "kernels.h"
using namespace bn;

BN_KERNEL k_hash_to_g1_x(uint32_t xid, const uint8_t* msgs, const uint64_t* off, size_t n, const uint8_t* dst, uint32_t dst_len,
                         int32_t* h_ws, size_t h_stride, uint8_t* out_bytes, int mode) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t* m = msgs + off[i];
  size_t len = (size_t)(off[i + 1] - off[i]);
  if (mode == 3) {            // homogeneous (X : Y : Z), 27 limbs, for the table-only Miller loop
    G1P hp = lane_hash_to_g1_proj_x(xid, m, len, dst, dst_len);
    store_fp(h_ws + i, h_stride, hp.x); store_fp(h_ws + 9 * h_stride + i, h_stride, hp.y); store_fp(h_ws + 18 * h_stride + i, h_stride, hp.z);
    return;
  }
  G1A h = mode == 2 ? lane_encode_to_g1_x(xid, m, len, dst, dst_len) : lane_hash_to_g1_x(xid, m, len, dst, dst_len);
  if (mode == 0) { store_fp(h_ws + i, h_stride, h.x); store_fp(h_ws + 9 * h_stride + i, h_stride, h.y); }
  else g1_encode(out_bytes + 64 * i, h);
}
BN_KERNEL_1 k_hash_to_g2_x(uint32_t xid, const uint8_t* msgs, const uint64_t* off, size_t n, const uint8_t* dst, uint32_t dst_len,
                           uint8_t* out_bytes, int ro) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  g2_encode(out_bytes + 128 * i, lane_hash_to_g2_x(xid, msgs + off[i], (size_t)(off[i + 1] - off[i]), dst, dst_len, ro != 0));
}
// sig = [sk] H(msg): the double-and-add of k_sign behind the hash under xid.  Scalars: 32 bytes big-endian, must be < r
BN_KERNEL_1 k_sign_x(uint32_t xid, const uint8_t* sks, const uint8_t* msgs, const uint64_t* off, size_t n, const uint8_t* dst, uint32_t dst_len,
                     uint8_t* sigs, uint8_t* status) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t* sk = sks + 32 * i;
  bool ok;
  (void)fr_from_be(sk, ok);                      // range check against r
  uint64_t k[4];
  for (int w = 0; w < 4; ++w) {
    uint64_t v = 0;
    for (int j = 0; j < 8; ++j) v = (v << 8) | sk[8 * (3 - w) + j];
    k[w] = v;
  }
  G1A h = lane_hash_to_g1_x(xid, msgs + off[i], (size_t)(off[i + 1] - off[i]), dst, dst_len);
  g1_encode(sigs + 64 * i, g1_to_affine(proj_mul_256(proj_from_affine(h), k)));
  status[i] = ok ? 1 : 0;
}
BN_KERNEL k_hash_to_scalar_x(uint32_t xid, const uint8_t* msgs, const uint64_t* off, size_t n, const uint8_t* dst, uint32_t dst_len, uint8_t* out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fr_to_be(out + 32 * i, lane_hash_to_scalar_x(xid, msgs + off[i], (size_t)(off[i + 1] - off[i]), dst, dst_len));
}
