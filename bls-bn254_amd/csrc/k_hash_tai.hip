// k_hash_tai.hip -- the hashing kernels under the try-and-increment map to G1 (lane_hash_tai.h; blsbn254_set_g1_map, DESIGN.md
// 6u): the siblings of k_hash_to_g1 (k_hash_g1.hip) and k_sign (k_sign.hip), which stay as they are.  The host launches these
// when the context's map is not SVDW (host_common.h launch_hash_to_g1 / launch_sign).  Same arguments, workspace layouts and
// modes as the SVDW kernels (mode 2, encode, never comes here), plus the map id and the expander id; dst is accepted and ignored.
// Own translation unit under k_hash_g1.hip's policy (-DBN_FORCE_INLINE, two waves per SIMD).
//
// The search has a trip count that depends on the data: half of all x have a square x^3 + 3, so a message needs 2 candidates on
// average, but a wave waits for the slowest of its 64 lanes.  Two forms, ONE compiled in: the pooled one, which the measurement
// of DESIGN.md 6u chose (the hash launch in 0.58 of the plain form's time); -DTAI_PLAIN builds the other for that measurement.
//   plain   every lane walks its own candidates (tai_search); the wave leaves with its last lane: 7.3 rounds on average.
//   pooled  the wave owns its 64 messages together: 3.4 rounds on average.  Round 1: every lane tests candidate 0 of its own
//           message.  Every later round: the u messages still open get per = floor(64 / u) lanes each, lane L testing candidate
//           done + L % per of the message of rank L / per among the open ones, where `done` candidates per open message are
//           known non-residues (the same count for all of them: every round gives each the same number of lanes).  x travels
//           by __shfl, the verdicts by __ballot; a message's winner is the lowest set bit of its segment of the ballot, so the
//           smallest k wins and the result is the sequential one.  Lanes past n take part as helpers that own nothing.
#include "lane_hash_tai.h"
#include "fr29.h"
#include "kernels.h"
using namespace bn;

#ifndef TAI_PLAIN
// the lane of the j-th set bit of m (j < popcount(m)): binary search over the popcounts of the low halves
__device__ inline uint32_t nth_set_lane(uint64_t m, uint32_t j) {
  uint32_t base = 0;
  BN_UNROLL for (uint32_t w = 32; w; w >>= 1) {
    const uint32_t c = (uint32_t)__popcll(m & ((1ull << w) - 1));
    const bool up = j >= c;
    j -= up ? c : 0; base += up ? w : 0; m = up ? m >> w : m;
  }
  return base;
}
// x: the lane's x0 (any value for a lane that owns no message: own = false).  Returns whether the lane's message found its
// winner, k its distance from x0.  Wave-uniform control flow around every __shfl and __ballot.
__device__ inline bool tai_search_pooled(const Fp& x0, bool own, uint32_t& k) {
  const uint32_t lane = threadIdx.x & 63;
  bool open = own;
  if (open) open = !fp_is_square(tai_rhs(x0));
  k = 0;
  uint32_t done = 1;
  uint64_t U = __ballot(open);
  while (U != 0 && done < (uint32_t)TAI_CAP) {
    const uint32_t u = (uint32_t)__popcll(U), per = 64 / u;
    const uint32_t j = lane / per, cand = done + lane % per;
    const bool work = j < u && cand < (uint32_t)TAI_CAP;
    const uint32_t src = nth_set_lane(U, j < u ? j : 0);
    Fp xm;
    BN_UNROLL for (int t = 0; t < NL; ++t) xm.l[t] = __shfl(x0.l[t], (int)src, 64);
    bool sq = false;
    if (work) sq = fp_is_square(tai_rhs(tai_offset(xm, cand)));
    const uint64_t B = __ballot(sq);
    if (open) {
      const uint32_t rank = (uint32_t)__popcll(U & ((1ull << lane) - 1));
      const uint64_t seg = (B >> (rank * per)) & (per == 64 ? ~0ull : (1ull << per) - 1);
      if (seg) { open = false; k = done + (uint32_t)__builtin_ctzll(seg); }
    }
    done += per;
    U = __ballot(open);
  }
  return own && !open;
}
#endif

// the lane's point: x0, the search in the form the unit is built with, one root
__device__ inline G1A tai_lane_point(uint32_t map, uint32_t xid, const uint8_t* msgs, const uint64_t* off, size_t i, size_t n) {
#ifndef TAI_PLAIN
  const bool own = i < n;
  Fp x0 = fp_zero();
  if (own) x0 = tai_x0(map, xid, msgs + off[i], (size_t)(off[i + 1] - off[i]));
  uint32_t k;
  const bool found = tai_search_pooled(x0, own, k);
  if (!own) { G1A z; z.x = fp_zero(); z.y = fp_zero(); z.inf = false; return z; }
  return tai_point(tai_offset(x0, k), found);
#else
  if (i >= n) { G1A z; z.x = fp_zero(); z.y = fp_zero(); z.inf = false; return z; }
  return lane_hash_to_g1_tai(map, xid, msgs + off[i], (size_t)(off[i + 1] - off[i]));
#endif
}

BN_KERNEL k_hash_to_g1_tai(uint32_t map, uint32_t xid, const uint8_t* msgs, const uint64_t* off, size_t n, const uint8_t* dst, uint32_t dst_len,
                           int32_t* h_ws, size_t h_stride, uint8_t* out_bytes, int mode) {
  (void)dst; (void)dst_len;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const G1A h = tai_lane_point(map, xid, msgs, off, i, n);
  if (i >= n) return;
  if (mode == 1) { g1_encode(out_bytes + 64 * i, h); return; }
  store_fp(h_ws + i, h_stride, h.x); store_fp(h_ws + 9 * h_stride + i, h_stride, h.y);
  if (mode == 3) store_fp(h_ws + 18 * h_stride + i, h_stride, fp_one());      // homogeneous (x : y : 1) for the table-only Miller loop
}
// sig = [sk] H(msg): the double-and-add of k_sign behind the map.  Scalars: 32 bytes big-endian, must be < r
BN_KERNEL_1 k_sign_tai(uint32_t map, uint32_t xid, const uint8_t* sks, const uint8_t* msgs, const uint64_t* off, size_t n, const uint8_t* dst, uint32_t dst_len,
                       uint8_t* sigs, uint8_t* status) {
  (void)dst; (void)dst_len;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const G1A h = tai_lane_point(map, xid, msgs, off, i, n);
  if (i >= n) return;
  const uint8_t* sk = sks + 32 * i;
  bool ok;
  (void)fr_from_be(sk, ok);                      // range check against r
  uint64_t k[4];
  for (int w = 0; w < 4; ++w) {
    uint64_t v = 0;
    for (int j = 0; j < 8; ++j) v = (v << 8) | sk[8 * (3 - w) + j];
    k[w] = v;
  }
  g1_encode(sigs + 64 * i, g1_to_affine(proj_mul_256(proj_from_affine(h), k)));
  status[i] = ok ? 1 : 0;
}
