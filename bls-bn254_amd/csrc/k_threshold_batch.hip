// k_threshold_batch.hip -- threshold combine over MANY groups in one call (threshold_batch.h; host_threshold_batch.hip):
// one lane per SHARE over all groups of a launch.
//   k_fr_decode          (k_threshold.hip) ids -> Montgomery limbs, validity
//   k_lagrange_seg       lane i: its group by binary search in the offsets, both length-t products of lambda_i over the group,
//                        one inversion, canonical bytes (when asked for) and the GLV halves in the th_glv layout
//   k_g1_smul_glv        lane i: decode + curve equation, [k1] P + [k2] phi(P) on one chain of 126 doublings with the table
//                        {P, 3P, 5P, 7P} in the lane's LDS column; the product stays homogeneous (no inversion, no bytes)
//   k_g1_seg_sum         (k_rlc2.hip) the products of each group summed level by level
//   k_g1p_to_bytes       (k_rlc.hip) one inversion per GROUP
//   k_th_finish          per group: the marks the lanes left -> status; a bad group's bytes become the identity encoding
// Shares of a group larger than t_big (the host sends those through the single-group pipeline of k_threshold.hip) only get the
// point check here.
#include "threshold_batch.h"
#include "kernels.h"
#include "../../include/blsbn254.h"
using namespace bn;

// Launch of m shares = shares lo .. lo + m of the call; goff[0 .. ng]: the offsets of the launch's groups in the call's
// numbering (goff[0] <= lo, lo + m <= goff[ng]; only a group above t_big may reach beyond the launch).
// gid[i] = the lane's group (index into goff) | TH_GID_BIG; gstat[g] bit 0: a bad or repeated id in group g.
BN_KERNEL k_lagrange_seg(const int32_t* x_ws, const uint8_t* id_ok, size_t m, uint32_t lo, const uint32_t* goff, uint32_t ng, uint32_t t_big,
                         uint8_t* scalars, uint32_t* glv_ws, uint32_t* gid, uint32_t* gstat) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint32_t g = th_find_group(goff, ng, lo + (uint32_t)i);
  const uint32_t a = goff[g], b = goff[g + 1];
  const bool big = b - a > t_big;
  gid[i] = g | (big ? TH_GID_BIG : 0u);
  if (big) return;
  bool bad;
  const Fr lam = lagrange_seg_lane(x_ws, id_ok, m, (uint32_t)i, a - lo, b - lo, bad);
  if (bad) atomicOr(gstat + g, 1u);
  uint32_t w[8];
  th_fr_words(lam, w);
  if (scalars) for (int j = 0; j < 8; ++j) store_be32(scalars + 32 * i + 4 * (7 - j), w[j]);
  const GlvSplit s = glv_split(w);
  for (int j = 0; j < 4; ++j) { glv_ws[(size_t)j * m + i] = s.k1[j]; glv_ws[(size_t)(4 + j) * m + i] = s.k2[j]; }
  glv_ws[(size_t)8 * m + i] = (s.neg1 ? 1u : 0u) | (s.neg2 ? 2u : 0u);
}
// out_ws: 27 x m limbs, limb-major homogeneous points (canonical limbs).  gstat[g] bit 1: a share of group g does not decode
// or is off the curve.
BN_KERNEL k_g1_smul_glv(const uint8_t* g1, const uint32_t* glv_ws, const uint32_t* gid, size_t m, int32_t* out_ws, uint32_t* gstat) {
  __shared__ int32_t lds[TH_SMUL_TAB_LIMBS * 256];     // each lane touches only its own column: no barrier needed
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  bool ok;
  const G1A p = th_point(g1 + 64 * i, ok);
  const uint32_t gw = gid[i];
  if (!ok) atomicOr(gstat + (gw & ~TH_GID_BIG), 2u);
  if (gw & TH_GID_BIG) return;
  GlvSplit s;
  for (int j = 0; j < 4; ++j) { s.k1[j] = glv_ws[(size_t)j * m + i]; s.k2[j] = glv_ws[(size_t)(4 + j) * m + i]; }
  const uint32_t fl = glv_ws[(size_t)8 * m + i];
  s.neg1 = (fl & 1u) != 0; s.neg2 = (fl & 2u) != 0;
  const G1P r = g1_smul_glv_lane(p, s, Ws{lds, 256, threadIdx.x * 4u, false});
  store_fp(out_ws + i, m, r.x); store_fp(out_ws + 9 * m + i, m, r.y); store_fp(out_ws + 18 * m + i, m, r.z);
}
// status[g] = BLSBN254_ERR_SCALAR / BLSBN254_ERR_G1 / 0 (scalar errors take precedence, as in the single call); out (optional):
// the groups' 64-byte encodings, a bad group's replaced by the identity (0, 1)
__global__ void __launch_bounds__(256) k_th_finish(const uint32_t* gstat, size_t n_groups, uint8_t* out, uint8_t* status) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups) return;
  const uint32_t st = gstat[g];
  const uint8_t code = (st & 1u) ? BLSBN254_ERR_SCALAR : (st & 2u) ? BLSBN254_ERR_G1 : 0;
  status[g] = code;
  if (code && out) for (int b = 0; b < 64; ++b) out[64 * g + b] = b == 63 ? 1 : 0;
}
