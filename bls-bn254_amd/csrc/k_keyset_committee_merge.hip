// k_keyset_committee_merge.hip -- the selection kernel of the checked merge of partial aggregates PER COMMITTEE of a registered
// key set (keyset_committee_merge.h has the lane functions; host_keyset_committee_merge.hip):
//   k_kcm_select       k_km_select over RAGGED rows: ONE WAVE per group, lane l owning the 32-member words l, l + 64, ... of every
//                      row of its group.  The width of the rows comes from the record of the group's committee, the validity
//                      words are the committee's own (cvalid at its word base), the contribution rows lie back to back from the
//                      group's byte offset and the merged row at the byte offset the caller's sel_off gives it.  The wave walks
//                      its group's contributions in the order given, takes three votes per contribution (row not empty, row
//                      within the valid members, row disjoint from the union so far) and, where the signature byte of the
//                      EARLIER launch, the mask bit and the votes agree, ORs the row into the union; lane 0 writes the
//                      contribution's byte (KM_CAND | KM_USED).  The union is the group's merged row: one register per lane for
//                      a committee of up to 2048 members, the merged row itself above that.  Launches end on group boundaries
//   k_km_sig, k_km_points (k_keyset_merge.hip) the signature test and the bitmaps, per contribution; k_g1_seg_sum, k_g1p_to_bytes
//   (k_rlc2.hip, k_rlc.hip) the groups' signature sums; k_kc_* (k_keyset_committee.hip) the key sums from the merged rows
// No member index is gathered and no registry-wide word is read.  Apart from the votes no lane reads another lane's result of
// its launch.  Plain vector stores, no atomics.
#include "keyset_committee_merge.h"
#include "kernels.h"
using namespace bn;

// Launch of m groups = groups g_lo .. g_lo + m of the call, four waves (groups) per workgroup.  goff[0 .. n_groups]: the groups'
// contribution offsets rebased to 0; com: the groups' committees; coms / cvalid: the handle's table; rbase / roff: the byte
// offsets of the groups' first contribution row in rows and of their merged row in urows.  mask: a bitmap over the call's
// contributions or null (all ones); flags: a byte per contribution.
__global__ void __launch_bounds__(256) k_kcm_select(const uint8_t* rows, const uint8_t* sig_ok, const uint8_t* mask, const uint32_t* goff, const uint32_t* com,
                                                   const uint4* coms, const uint32_t* cvalid, const uint64_t* rbase, const uint64_t* roff, size_t g_lo, size_t m,
                                                   uint8_t* flags, uint8_t* urows) {
  const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (wave >= m) return;                                 // the whole wave
  const uint32_t lane = threadIdx.x & 63;
  const size_t g = g_lo + wave;
  const uint4 k = coms[com[g]];                          // off, size, wbase
  const KcmGroup v = kcm_group(k.y, k.z, cvalid, goff, rbase, roff, g, rows, urows);
  uint32_t ureg;
  km_begin(v.urow, v.rb, v.W, lane, ureg);
#pragma unroll 1
  for (uint32_t s = v.a; s < v.b; ++s) {
    const uint8_t* row = kcm_row(v, s);
    const KmVote t = km_test(row, v.rb, v.W, lane, v.valid, v.urow, ureg);
    const KmVote any{__any(t.some) != 0, __any(t.invalid) != 0, __any(t.overlap) != 0};
    const uint8_t f = km_flags(sig_ok[s] != 0, mask ? tc_bit(mask, s) : true, any);
    if (f & KM_USED) km_take(row, v.rb, v.W, lane, v.urow, ureg);
    if (lane == 0) flags[s] = f;
  }
  km_end(v.urow, v.rb, v.W, lane, ureg);
}
