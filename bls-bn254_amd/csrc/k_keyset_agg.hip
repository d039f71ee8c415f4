// k_keyset_agg.hip -- the selection kernels of the checked signature aggregation over a registered key set (keyset_agg.h has
// the lane functions; host_keyset_agg.hip):
//   k_ka_scan          lane i: the candidate bit of its entry into the call's candidate bitmap (by ballot), its signature as a
//                      projective point into the limb-major workspace the segmented G1 sum reads, the identity for a non-candidate
//   k_ka_rows          one lane per (group, 32-key word): the word of the group's participation row from the candidate bits,
//                      stored as bytes (a row is ceil(n_keys / 8) bytes, in general no multiple of 4)
//   k_ka_gather_keys   the fallback only: the 128-byte encoding of every entry's key, copied by index, eight lanes per entry
//   k_g1_seg_sum, k_g1p_to_bytes (k_rlc2.hip, k_rlc.hip) the groups' signature sums; k_ks_* (k_keyset.hip) the key sums from the rows
// An entry depends on no other lane's result of its launch, so a launch may end anywhere; the candidate bitmap is complete once
// every launch of k_ka_scan has run, which is why k_ka_rows is a pass of its own.  Plain vector stores, no atomics.
#include "keyset_agg.h"
#include "kernels.h"
using namespace bn;

// Launch of m entries = entries lo .. lo + m of the call's N (lo a multiple of 8).  idx / sigs / mask / cand / pts: the call's.
BN_KERNEL k_ka_scan(const uint8_t* key_valid, const uint32_t* idx, const uint8_t* sigs, const uint8_t* mask, size_t m, uint32_t lo, size_t N, uint8_t* cand,
                    int32_t* pts) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool c = false;
  if (i < m) {
    const size_t s = (size_t)lo + i;
    const KaScan r = ka_scan(key_valid, idx, sigs, mask, s);
    c = r.cand;
    ka_store_point(pts + s, N, r.p);
  }
  write_ballot(cand + (lo >> 3), m, i, c);
}
// Launch of m lanes = lanes lo .. lo + m of the call's n_groups x W, lane t = word t % W of group t / W.  goff[0 .. n_groups]:
// the groups' entry offsets rebased to 0.  rows: n_groups rows of ceil(n_keys / 8) bytes.
__global__ void __launch_bounds__(256) k_ka_rows(const uint32_t* idx, const uint8_t* cand, const uint32_t* goff, size_t m, size_t lo, uint32_t n_keys, uint8_t* rows) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const size_t t = lo + i;
  const uint32_t W = ks_words(n_keys), rb = ks_row_bytes(n_keys);
  const size_t g = t / W;
  const uint32_t w = (uint32_t)(t - g * W);
  ka_row_store(rows + g * rb, rb, w, ka_row_word(idx, cand, goff[g], goff[g + 1], w));
}
// enc: the key set's encodings, 8 x 16 bytes per key; out[8 e + q] = piece q of the key of entry e, e < m.  A lane holds one
// 16-byte piece in registers.
__global__ void __launch_bounds__(256) k_ka_gather_keys(const uint4* enc, const uint32_t* idx, size_t m, uint4* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 8 * m) return;
  out[i] = enc[8 * (size_t)idx[i >> 3] + (i & 7)];
}
