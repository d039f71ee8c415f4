// k_keyset_merge.hip -- the selection kernels of the checked merge of partial aggregates over a registered key set
// (keyset_merge.h has the lane functions; host_keyset_merge.hip):
//   k_km_sig           lane i: the signature test of its contribution as one BYTE, its signature as a projective point into the
//                      limb-major workspace the segmented G1 sum reads
//   k_km_select        ONE WAVE per group, lane l owning the 32-key words l, l + 64, ... of every row: the wave walks its
//                      group's contributions in the order given, takes three votes per contribution (row not empty, row within
//                      the valid keys, row disjoint from the union so far) and, where the signature byte of the EARLIER launch,
//                      the mask bit and the votes agree, ORs the row into the union; lane 0 writes the contribution's byte
//                      (KM_CAND | KM_USED).  The union is the group's merged row.  Launches end on group boundaries
//   k_km_points        lane i: the identity over the point of a contribution that is not used, and the bytes of the select
//                      launches packed into the call's used and candidate bitmaps (by ballot: bytes at the launch edges)
//   k_g1_seg_sum, k_g1p_to_bytes (k_rlc2.hip, k_rlc.hip) the groups' signature sums; k_ks_* (k_keyset.hip) the key sums from the rows
// Apart from the votes no lane reads another lane's result of its launch: k_km_select reads the bytes k_km_sig wrote, k_km_points
// the bytes k_km_select wrote.  Plain vector stores, no atomics.
#include "keyset_merge.h"
#include "kernels.h"
using namespace bn;

// Launch of m contributions = contributions lo .. lo + m of the call's N.  sigs / sig_ok / pts: the call's.
BN_KERNEL k_km_sig(const uint8_t* sigs, size_t m, uint32_t lo, size_t N, uint8_t* sig_ok, int32_t* pts) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const size_t s = (size_t)lo + i;
  const KmSig r = km_sig(sigs, s);
  sig_ok[s] = r.ok ? 1 : 0;
  ka_store_point(pts + s, N, r.p);
}
// Launch of m groups = groups g_lo .. g_lo + m of the call, four waves (groups) per workgroup.  goff[0 .. n_groups]: the groups'
// contribution offsets rebased to 0.  rows: the call's N rows of ceil(n_keys / 8) bytes; mask: a bitmap over the call's
// contributions or null (all ones); valid: the key set's KeyValidate bits by words; flags: a byte per contribution; urows:
// n_groups merged rows.
__global__ void __launch_bounds__(256) k_km_select(const uint8_t* rows, const uint8_t* sig_ok, const uint8_t* mask, const uint32_t* goff, const uint32_t* valid,
                                                  uint32_t n_keys, size_t g_lo, size_t m, uint8_t* flags, uint8_t* urows) {
  const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (wave >= m) return;                                 // the whole wave
  const uint32_t lane = threadIdx.x & 63;
  const size_t g = g_lo + wave;
  const uint32_t W = ks_words(n_keys), rb = ks_row_bytes(n_keys);
  uint8_t* urow = urows + g * rb;
  uint32_t ureg;
  km_begin(urow, rb, W, lane, ureg);
  const uint32_t a = goff[g], b = goff[g + 1];
#pragma unroll 1
  for (uint32_t s = a; s < b; ++s) {
    const uint8_t* row = rows + (size_t)s * rb;
    const KmVote v = km_test(row, rb, W, lane, valid, urow, ureg);
    const KmVote any{__any(v.some) != 0, __any(v.invalid) != 0, __any(v.overlap) != 0};
    const uint8_t f = km_flags(sig_ok[s] != 0, mask ? tc_bit(mask, s) : true, any);
    if (f & KM_USED) km_take(row, rb, W, lane, urow, ureg);
    if (lane == 0) flags[s] = f;
  }
  km_end(urow, rb, W, lane, ureg);
}
// Launch of m contributions = contributions lo .. lo + m of the call's N (lo a multiple of 8).
BN_KERNEL k_km_points(const uint8_t* flags, size_t m, uint32_t lo, size_t N, int32_t* pts, uint8_t* used, uint8_t* cand) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool u = false, c = false;
  if (i < m) {
    const size_t s = (size_t)lo + i;
    const uint8_t f = flags[s];
    u = (f & KM_USED) != 0; c = (f & KM_CAND) != 0;
    if (!u) km_drop_point(pts + s, N);
  }
  write_ballot(used + (lo >> 3), m, i, u);
  write_ballot(cand + (lo >> 3), m, i, c);
}
