// k_threshold_checked.hip -- the selection kernels of the checked threshold combine over MANY groups (threshold_checked.h;
// host_threshold_checked.hip): one lane per SHARE over all groups of a call, one lane per GROUP for the keys.
//   k_g2_load, k_g2_check (k_groupops.hip, k_g2_check.hip) the commitments, once per call
//   k_fr_decode          (k_threshold.hip) ids -> validity (decodes and non-zero)
//   k_tc_scan            lane i: the candidate bit of its partial signature into the call's candidate bitmap; a bad id, or one
//                        that an earlier share of the group already has, marks the group
//   k_td_finish          (k_threshold_deal.hip) the commitments' validity bytes folded into the marks
//   k_tc_select          lane i: its rank among the set bits of its group; the first t_g set shares of an unmarked group with
//                        at least t_g of them go to slot coff[g] + rank of the compacted ids / partial signatures and get
//                        their used bit; a group with too few gets the short mark
//   k_lagrange_seg .. k_th_finish (k_threshold_batch.hip) the combine over the compacted arrays
//   k_tc_gather_c0       per group: C_0 as the key of the group's ONE verification, the identity for a group that carries a mark
// A share depends on no other lane's result, only on its group's inputs, so a launch may end anywhere; the marks of a group
// are complete once every launch of k_tc_scan has run, which is why k_tc_select is a pass of its own.
#include "threshold_checked.h"
#include "kernels.h"
#include "../../include/blsbn254.h"
using namespace bn;

// Launch of m shares = shares lo .. lo + m of the call's N (lo a multiple of 8); goff[0 .. ng]: the id offsets of ALL groups
// of the call, rebased to 0.  ids / sigs: the call's; id_ok: the launch's (k_fr_decode); cand: the call's bitmap.
BN_KERNEL k_tc_scan(const uint8_t* ids, const uint8_t* sigs, const uint8_t* id_ok, size_t m, uint32_t lo, const uint32_t* goff, uint32_t ng, uint32_t* gstat,
                    uint8_t* cand) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool c = false;
  if (i < m) {
    const uint32_t s = lo + (uint32_t)i;
    const uint32_t g = th_find_group(goff, ng, s);
    c = tc_candidate(sigs + 64 * (size_t)s);
    if (!(id_ok[i] & 1) | tc_repeats(ids, goff[g], s)) atomicOr(gstat + g, TD_MARK_SCALAR);
  }
  write_ballot(cand + (lo >> 3), m, i, c);
}
// bits_a AND bits_b (null: all ones): bitmaps over the call's shares.  gstat: complete as far as ids and commitments go.
// c_ids / c_sigs: the compacted arrays, coff[ng] slots, zeroed by the host (a group that is not picked keeps zero ids, which
// the combine marks, and its output is the identity).  used: the call's bitmap.
__global__ void __launch_bounds__(256) k_tc_select(const uint8_t* bits_a, const uint8_t* bits_b, size_t m, uint32_t lo, const uint32_t* goff, const uint32_t* coff,
                                                  uint32_t ng, uint32_t* gstat, const uint32_t* ids, const uint32_t* sigs, uint32_t* c_ids, uint32_t* c_sigs,
                                                  uint8_t* used) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool u = false;
  if (i < m) {
    const uint32_t s = lo + (uint32_t)i;
    const uint32_t g = th_find_group(goff, ng, s);
    const uint32_t a = goff[g], t = coff[g + 1] - coff[g];
    const TcRank r = tc_rank(bits_a, bits_b, a, goff[g + 1], s);
    if ((s == a) & tc_short(r, t)) atomicOr(gstat + g, TC_MARK_SHORT);
    u = tc_pick(r, t, gstat[g]);
    if (u) {
      const size_t slot = (size_t)coff[g] + r.rank;
      for (int k = 0; k < 8; ++k) c_ids[8 * slot + k] = ids[8 * (size_t)s + k];
      for (int k = 0; k < 16; ++k) c_sigs[16 * slot + k] = sigs[16 * (size_t)s + k];
    }
  }
  write_ballot(used + (lo >> 3), m, i, u);
}
// commitments: the call's, 128 B each; keys[128 g ..] = C_0 of group g.  A group too small for its threshold (an empty one has
// no lane in k_tc_select) gets its short mark here; a marked group's key is the identity encoding, which no verification accepts.
__global__ void __launch_bounds__(256) k_tc_gather_c0(const uint32_t* commitments, const uint32_t* coff, const uint32_t* goff, size_t n_groups, uint32_t* gstat,
                                                     uint32_t* keys) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups) return;
  const uint32_t t = coff[g + 1] - coff[g];
  uint32_t st = gstat[g];
  if ((t == 0) | (goff[g + 1] - goff[g] < t)) { st |= TC_MARK_SHORT; gstat[g] = st; }
  if (st != 0) {                                         // (0, 1): byte 127 is the last byte of little-endian word 31
    for (int k = 0; k < 32; ++k) keys[32 * g + k] = k == 31 ? 0x01000000u : 0u;
  } else {
    const uint32_t* src = commitments + 32 * (size_t)coff[g];
    for (int k = 0; k < 32; ++k) keys[32 * g + k] = src[k];
  }
}
