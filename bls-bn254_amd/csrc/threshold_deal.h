// threshold_deal.h -- what ONE lane does on the dealing side of the threshold scheme (k_threshold_deal.hip,
// host_threshold_deal.hip): one lane per SHARE, group g owning the ids goff[g] .. goff[g + 1] and the polynomial
// coefficients (or their Feldman commitments C_j = [a_j] G2gen) coff[g] .. coff[g + 1], low order first.
//     share_i  = f_g(x_i)        = sum_j a_j x_i^j          (Scalar multiply / add, scalar.rs:523-548)
//     pk_i     = [f_g(x_i)] G2   = sum_j [x_i^j] C_j        (Mul<Scalar> g2.rs:866-886, Add g2.rs:789-831)
// both by Horner from the highest coefficient down, so neither needs a power of x_i nor an inversion.
//   fr_horner_lane       acc = acc x + a_j in Montgomery form; every lane of a group reads the same coefficient address
//   g2_horner_lane       acc = [x] acc + C_j; [x] acc is plain double-and-add over the complete RCB formulas with proj_select
//                        for the bit, over `nbits` bits -- ONE value per launch (the largest bit length of the launch's ids),
//                        so no lane branches on its data and small participant ids cost what their width costs
// tests/hostsim/threshold_deal_host.cpp runs the same functions on the host with -DBN_CHECK (interval discipline) against
// the oracle.  They are not a CPU fallback: nothing in the product's host path calls them.
#pragma once
#include "threshold_batch.h"

namespace bn {

constexpr uint32_t TD_MARK_SCALAR = 1u;          // gstat bit: an id of the group is >= r or 0, or a coefficient is >= r
constexpr uint32_t TD_MARK_POINT = 2u;           // gstat bit: a commitment of the group does not decode / is off the curve / outside the subgroup
constexpr int TD_MAX_BITS = 254;                 // bit length of r - 1

BN_INL G2P td_load_g2p(const int32_t* ws, size_t stride) {
  return {{load_fp(ws, stride), load_fp(ws + 9 * stride, stride)},
          {load_fp(ws + 18 * stride, stride), load_fp(ws + 27 * stride, stride)},
          {load_fp(ws + 36 * stride, stride), load_fp(ws + 45 * stride, stride)}};
}
BN_INL void td_store_g2p(int32_t* ws, size_t stride, const G2P& p) {
  store_fp(ws, stride, p.x.c0); store_fp(ws + 9 * stride, stride, p.x.c1);
  store_fp(ws + 18 * stride, stride, p.y.c0); store_fp(ws + 27 * stride, stride, p.y.c1);
  store_fp(ws + 36 * stride, stride, p.z.c0); store_fp(ws + 45 * stride, stride, p.z.c1);
}
// 1 in Montgomery form when the lane's id is unusable, so that the arithmetic stays uniform and in range (the lane's
// result is discarded through its group's mark)
BN_INL Fr td_id_or_one(const Fr& x, bool ok) { return fr_select(ok, x, fr_const(bnc::FR_ONE)); }

// f(x) for the coefficients [a, b) of cf_ws (Montgomery limbs, limb-major, stride T); a == b: the zero polynomial
BN_FUNC Fr fr_horner_lane(const int32_t* cf_ws, size_t T, uint32_t a, uint32_t b, const Fr& x) {
  Fr acc; for (int k = 0; k < NL; ++k) acc.l[k] = 0;
#pragma unroll 1
  for (uint32_t j = b; j-- > a;) acc = fr_add(fr_mul(acc, x), th_load_fr(cf_ws + j, T));
  return acc;
}

// bit i (0 .. 255) of the canonical little-endian words k; i is uniform over the launch
BN_INL bool td_bit(const uint32_t* k, int i) {
  const int w = i >> 5;
  uint32_t v = 0;
  BN_UNROLL for (int j = 0; j < 8; ++j) v = j == w ? k[j] : v;
  return (v >> (i & 31)) & 1u;
}
// sum_j [x^j] C_j for the commitments [a, b) of c_ws (homogeneous, limb-major, stride T; every one ON THE CURVE or the
// identity), x = the canonical words k, all of whose bits lie below nbits.  (b - a - 1) x (2 nbits + 1) group operations;
// a == b: the identity.  The result stays homogeneous (the inversion and the bytes come after the last launch, when the
// group's marks are complete).
BN_FUNC G2P g2_horner_lane(const int32_t* c_ws, size_t T, uint32_t a, uint32_t b, const uint32_t* k, int nbits) {
  BN_CTX;
  G2P acc = proj_identity<Fp2>();
  if (a == b) return acc;
  acc = td_load_g2p(c_ws + (b - 1), T);
#pragma unroll 1
  for (uint32_t j = b - 1; j-- > a;) {
    G2P r = proj_identity<Fp2>();
#pragma unroll 1
    for (int i = nbits - 1; i >= 0; --i) {
      r = proj_dbl(r);
      const G2P s = proj_add(r, acc);
      r = proj_select(td_bit(k, i), s, r);
    }
    acc = proj_add(r, td_load_g2p(c_ws + j, T));
  }
  return acc;
}

}  // namespace bn
