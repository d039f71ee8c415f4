// k_keyset_committee_agg.hip -- the selection kernels of the checked signature aggregation per COMMITTEE of a registered key set
// (keyset_committee_agg.h has the lane functions; host_keyset_committee_agg.hip):
//   k_kca_scan         lane i: its entry's group by binary search in the entry offsets, then the candidate bit -- the bit of the
//                      entry's POSITION in the committee's validity words, the signature test, the optional mask -- into the call's
//                      candidate bitmap (by ballot), and its signature as a projective point into the limb-major workspace the
//                      segmented G1 sum reads, the identity for a non-candidate.  No member index is read
//   k_kca_rows         one lane per (group, 32-member word of its committee): the word lanes are RAGGED, a lane finds its group by
//                      binary search in the prefix of the groups' words; the word from the candidate bits (ka_row_word on
//                      positions), stored as bytes at the row's byte offset (a row is ceil(size / 8) bytes, unaligned)
//   k_kca_resolve      the fallback only: the registry index of every entry, members[first member + position]; k_ka_gather_keys
//                      (k_keyset_agg.hip) then copies the keys' encodings by those indices, unchanged
//   k_g1_seg_sum, k_g1p_to_bytes (k_rlc2.hip, k_rlc.hip) the groups' signature sums; k_kc_* (k_keyset_committee.hip) the key sums
//   from the rows
// An entry depends on no other lane's result of its launch, so a launch may end anywhere; the candidate bitmap is complete once
// every launch of k_kca_scan has run, which is why k_kca_rows is a pass of its own.  Plain vector stores, no atomics.
#include "keyset_committee_agg.h"
#include "kernels.h"
using namespace bn;

// Launch of m entries = entries lo .. lo + m of the call's N (lo a multiple of 8).  goff[0 .. ng]: the groups' entry offsets
// rebased to 0; com: the groups' committees; coms / cvalid: the handle's table.  pos / sigs / mask / cand / pts: the call's.
BN_KERNEL k_kca_scan(const uint32_t* cvalid, const uint4* coms, const uint32_t* com, const uint32_t* goff, uint32_t ng, const uint32_t* pos, const uint8_t* sigs,
                     const uint8_t* mask, size_t m, uint32_t lo, size_t N, uint8_t* cand, int32_t* pts) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool c = false;
  if (i < m) {
    const size_t s = (size_t)lo + i;
    const uint4 k = coms[com[kca_group(goff, ng, (uint32_t)s)]];          // off, size, wbase
    const KaScan r = kca_scan(cvalid + k.z, pos, sigs, mask, s);
    c = r.cand;
    ka_store_point(pts + s, N, r.p);
  }
  write_ballot(cand + (lo >> 3), m, i, c);
}
// Launch of m lanes = lanes lo .. lo + m of the call's wpre[ng] word lanes, lane t = word t - wpre[g] of the group g that owns
// it.  roff[g]: the byte offset of row g in rows.
__global__ void __launch_bounds__(256) k_kca_rows(const uint32_t* pos, const uint8_t* cand, const uint32_t* goff, const uint64_t* wpre, const uint64_t* roff,
                                                 const uint4* coms, const uint32_t* com, uint32_t ng, size_t m, uint64_t lo, uint8_t* rows) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint64_t t = lo + i;
  const uint32_t g = kca_word_group(wpre, ng, t);
  const uint32_t w = (uint32_t)(t - wpre[g]);
  ka_row_store(rows + roff[g], ks_row_bytes(coms[com[g]].y), w, ka_row_word(pos, cand, goff[g], goff[g + 1], w));
}
// Launch of m entries = entries lo .. lo + m of the call; idx: the call's resolved indices
__global__ void __launch_bounds__(256) k_kca_resolve(const uint32_t* members, const uint4* coms, const uint32_t* com, const uint32_t* goff, uint32_t ng,
                                                    const uint32_t* pos, size_t m, uint32_t lo, uint32_t* idx) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const size_t s = (size_t)lo + i;
  idx[s] = kca_resolve(members + coms[com[kca_group(goff, ng, (uint32_t)s)]].x, pos, s);
}
