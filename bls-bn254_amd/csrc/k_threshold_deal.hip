// k_threshold_deal.hip -- the dealing side of the threshold scheme over MANY groups in one call (threshold_deal.h;
// host_threshold_deal.hip): one lane per SHARE over all groups of a launch.
//   k_fr_decode          (k_threshold.hip) ids -> Montgomery limbs, validity (decodes and non-zero)
//   k_fr_coef_decode     lane j: coefficient j -> Montgomery limbs (limb-major, stride T) and a validity byte (< r)
//   k_fr_poly_eval       lane i: its group by binary search in the id offsets, Horner over the group's coefficients (all
//                        lanes of a group read the same coefficient address); the share stays in Montgomery form.  No inversion.
//   k_g2_load            (k_groupops.hip) commitments -> homogeneous limb-major workspace, once per call
//   k_g2_check           (k_g2_check.hip) decodes, on the curve, in the subgroup, once per call
//   k_g2_poly_eval       lane i: acc = C_{t-1}; acc = [id] acc + C_j by double-and-add over `nbits` bits (one value per launch);
//                        the key share stays homogeneous
//   k_td_finish          per group: the marks the lanes left and the validity bytes of the group's coefficients / commitments
//                        -> status (and the group's mark word, complete from here on)
//   k_td_fr_encode       lane i: canonical bytes of its share, zero bytes when its group carries a mark
//   k_td_g2_encode       lane i: ONE inversion per share, wire bytes; the identity encoding when its group carries a mark
// A lane's result can only be discarded once every lane of its group has run (the group may span launches), hence the two
// encode kernels after the last launch.
#include "threshold_deal.h"
#include "kernels.h"
#include "../../include/blsbn254.h"
using namespace bn;

BN_KERNEL k_fr_coef_decode(const uint8_t* coeffs, size_t T, int32_t* cf_ws, uint8_t* cf_ok) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= T) return;
  bool ok;
  const Fr a = fr_from_be(coeffs + 32 * j, ok);
  th_store_fr(cf_ws + j, T, a);
  cf_ok[j] = ok ? 1 : 0;
}
// Launch of m shares = shares lo .. lo + m of the call's N; goff / coff [0 .. ng]: the id and coefficient offsets of ALL groups
// of the call, rebased to 0 (goff[0] = 0 <= lo, lo + m <= goff[ng] = N).  x_ws / id_ok: the launch's decoded ids (stride m).
// r_ws: the call's shares, Montgomery limbs, limb-major, stride N.
BN_KERNEL k_fr_poly_eval(const int32_t* x_ws, const uint8_t* id_ok, size_t m, uint32_t lo, const uint32_t* goff, const uint32_t* coff, uint32_t ng,
                         const int32_t* cf_ws, size_t T, int32_t* r_ws, size_t N, uint32_t* gstat) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint32_t g = th_find_group(goff, ng, lo + (uint32_t)i);
  const bool ok = id_ok[i] & 1;
  if (!ok) atomicOr(gstat + g, TD_MARK_SCALAR);
  const Fr x = td_id_or_one(th_load_fr(x_ws + i, m), ok);
  th_store_fr(r_ws + lo + i, N, fr_horner_lane(cf_ws, T, coff[g], coff[g + 1], x));
}
// c_ws: the call's commitments, homogeneous, limb-major, stride T (an unusable one stored as the identity by k_g2_load).
// r_ws: the call's key shares, homogeneous, limb-major (54 x N limbs).
BN_KERNEL k_g2_poly_eval(const int32_t* x_ws, const uint8_t* id_ok, size_t m, uint32_t lo, const uint32_t* goff, const uint32_t* coff, uint32_t ng,
                         const int32_t* c_ws, size_t T, int nbits, int32_t* r_ws, size_t N, uint32_t* gstat) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint32_t g = th_find_group(goff, ng, lo + (uint32_t)i);
  const bool ok = id_ok[i] & 1;
  if (!ok) atomicOr(gstat + g, TD_MARK_SCALAR);
  uint32_t k[8];
  th_fr_words(td_id_or_one(th_load_fr(x_ws + i, m), ok), k);
  td_store_g2p(r_ws + lo + i, N, g2_horner_lane(c_ws, T, coff[g], coff[g + 1], k, nbits));
}
// shares lo .. lo + m of the call -> out (32 / 128 bytes per share of the launch); gstat complete (k_td_finish has run)
BN_KERNEL k_td_fr_encode(const int32_t* r_ws, size_t N, size_t m, uint32_t lo, const uint32_t* goff, uint32_t ng, const uint32_t* gstat, uint8_t* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const bool bad = gstat[th_find_group(goff, ng, lo + (uint32_t)i)] != 0;
  fr_to_be(out + 32 * i, fr_select(bad, Fr{}, th_load_fr(r_ws + lo + i, N)));
}
BN_KERNEL k_td_g2_encode(const int32_t* r_ws, size_t N, size_t m, uint32_t lo, const uint32_t* goff, uint32_t ng, const uint32_t* gstat, uint8_t* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const bool bad = gstat[th_find_group(goff, ng, lo + (uint32_t)i)] != 0;
  g2_encode(out + 128 * i, g2_to_affine(proj_select(bad, proj_identity<Fp2>(), td_load_g2p(r_ws + lo + i, N))));
}
// status[g] = BLSBN254_ERR_SCALAR / BLSBN254_ERR_G2 / 0 (scalar errors take precedence).  coff[0 .. n_groups]: the groups'
// coefficient offsets, rebased to 0.  ok_a (and ok_b, unless null): the validity bytes of the call's coefficients
// (k_fr_coef_decode) or commitments (k_g2_load, k_g2_check); a group with a failing one gets `mark`.
__global__ void __launch_bounds__(256) k_td_finish(uint32_t* gstat, size_t n_groups, const uint32_t* coff, const uint8_t* ok_a, const uint8_t* ok_b, uint32_t mark,
                                                  uint8_t* status) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups) return;
  uint32_t st = gstat[g];
  uint8_t all = 1;
  for (uint32_t j = coff[g]; j < coff[g + 1]; ++j) all &= ok_a[j] & (ok_b ? ok_b[j] : (uint8_t)1);
  if (!(all & 1)) st |= mark;
  gstat[g] = st;
  status[g] = (st & TD_MARK_SCALAR) ? BLSBN254_ERR_SCALAR : (st & TD_MARK_POINT) ? BLSBN254_ERR_G2 : 0;
}
