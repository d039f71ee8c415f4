// k_threshold_keycheck.hip -- dealt key shares checked against a group's Feldman commitments (threshold_keycheck.h;
// host_threshold_deal.hip): [s_i] G2gen == sum_j [id_i^j] C_j, one lane per SHARE over all groups of a call.
//   k_g2gen_table        once per context: lane w builds row w of the table of the generator's multiples (KC_WINDOWS lanes)
//   k_g2_poly_eval       (k_threshold_deal.hip, unchanged) the right-hand sides into the call's workspace, homogeneous
//   k_td_key_check       lane i: the share's range check, the fixed-base sum out of the table, proj_eq with its key share
//                        -> one byte per share.  No doubling, no inversion; the table is read through L2 (it is larger than LDS)
//   k_td_finish          (k_threshold_deal.hip, unchanged) the groups' marks, complete from here on, and statuses
//   k_td_key_bits        lane b: byte b of the bitmap = the bytes of its 8 shares, each ANDed with "its group carries no mark"
// The evaluation and the check stay two kernels: the evaluation already fills the register file.
#include "threshold_keycheck.h"
#include "kernels.h"
using namespace bn;

// tab: KC_TABLE_LIMBS limbs
__global__ void __launch_bounds__(64) k_g2gen_table(int32_t* tab) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= (uint32_t)KC_WINDOWS) return;
  kc_table_lane(tab, w);
}
// Launch of m shares = shares lo .. lo + m of the call's N (lo + m <= N).  shares: the call's N x 32 bytes; r_ws: the call's key
// shares (homogeneous, limb-major, stride N) as k_g2_poly_eval left them; share_ok: the call's N bytes.
BN_KERNEL k_td_key_check(const uint8_t* shares, size_t m, uint32_t lo, const int32_t* __restrict__ tab, const int32_t* r_ws, size_t N, uint8_t* share_ok) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const size_t s = lo + i;
  uint32_t k[8];
  bool ok;
  kc_share_words(shares + 32 * s, k, ok);
  share_ok[s] = kc_key_check_lane(tab, k, ok, td_load_g2p(r_ws + s, N)) ? 1 : 0;
}
// bitmap: ceil(N / 8) bytes, LSB-first, pad bits 0; gstat complete (k_td_finish has run); goff[0 .. ng]: the groups' id offsets
// rebased to 0 (goff[ng] = N > 0)
__global__ void __launch_bounds__(256) k_td_key_bits(const uint8_t* share_ok, size_t N, const uint32_t* goff, uint32_t ng, const uint32_t* gstat, uint8_t* bitmap) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= (N + 7) / 8) return;
  uint32_t v = 0;
  for (uint32_t j = 0; j < 8; ++j) {
    const size_t s = 8 * b + j;
    if (s < N && (share_ok[s] & 1) && gstat[th_find_group(goff, ng, (uint32_t)s)] == 0) v |= 1u << j;
  }
  bitmap[b] = (uint8_t)v;
}
