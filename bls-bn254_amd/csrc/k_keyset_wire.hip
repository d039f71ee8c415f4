// k_keyset_wire.hip -- the kernels of the checked aggregation and merge calls that speak wire format (32-byte signatures in and
// out; host_keyset_agg.hip, host_keyset_committee_agg.hip, host_keyset_merge.hip, host_keyset_committee_merge.hip):
//   k_ka_scan_wire     k_ka_scan (k_keyset_agg.hip) for 32-byte entries: lane i inflates its signature (g1_inflate_point: the
//                      fixed chain for the root, whose square test is the curve test) and goes on as k_ka_scan does -- the
//                      candidate bit by ballot, the point into the workspace of the segmented G1 sum.  No 64-byte form is stored
//   k_kca_scan_wire    k_kca_scan (k_keyset_committee_agg.hip) likewise
//   k_g1p_to_wire      a lane per group: the group's sum from its projective limbs as the 64 bytes the verify pipeline reads AND
//                      the 32 bytes the caller gets, one conversion to affine for both (ka_wire_out)
// The scans keep their siblings' rules: an entry depends on no other lane's result of its launch, so a launch may end anywhere;
// plain vector stores, no atomics.  Own translation unit, field functions force-inlined; the table of fp_pow_pm3_4 (14 field
// elements) lives in scratch, as in k_inflate.hip.
#include "keyset_committee_agg.h"
#include "kernels.h"
using namespace bn;

// Launch of m entries = entries lo .. lo + m of the call's N (lo a multiple of 8).  idx / sigs (32 B each) / mask / cand / pts: the call's.
BN_KERNEL k_ka_scan_wire(const uint8_t* key_valid, const uint32_t* idx, const uint8_t* sigs, const uint8_t* mask, size_t m, uint32_t lo, size_t N, uint8_t* cand,
                         int32_t* pts) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool c = false;
  if (i < m) {
    const size_t s = (size_t)lo + i;
    const KaScan r = ka_scan_wire(key_valid, idx, sigs, mask, s);
    c = r.cand;
    ka_store_point(pts + s, N, r.p);
  }
  write_ballot(cand + (lo >> 3), m, i, c);
}
// The same per committee: goff[0 .. ng], com, coms / cvalid as k_kca_scan takes them.
BN_KERNEL k_kca_scan_wire(const uint32_t* cvalid, const uint4* coms, const uint32_t* com, const uint32_t* goff, uint32_t ng, const uint32_t* pos, const uint8_t* sigs,
                          const uint8_t* mask, size_t m, uint32_t lo, size_t N, uint8_t* cand, int32_t* pts) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool c = false;
  if (i < m) {
    const size_t s = (size_t)lo + i;
    const uint4 k = coms[com[kca_group(goff, ng, (uint32_t)s)]];          // off, size, wbase
    const KaScan r = kca_scan_wire(cvalid + k.z, pos, sigs, mask, s);
    c = r.cand;
    ka_store_point(pts + s, N, r.p);
  }
  write_ballot(cand + (lo >> 3), m, i, c);
}
// ws: m sums, limb-major with the given stride.  full: 64 bytes per sum, wire: 32.
BN_KERNEL k_g1p_to_wire(const int32_t* ws, size_t stride, size_t m, uint8_t* full, uint8_t* wire) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  ka_wire_out(ka_load_point(ws + i, stride), full + 64 * i, wire + 32 * i);
}
