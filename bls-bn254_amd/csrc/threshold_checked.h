// threshold_checked.h -- what ONE lane does in the checked threshold combine over MANY groups (k_threshold_checked.hip,
// host_threshold_checked.hip): one lane per SHARE, group g owning the ids and partial signatures goff[g] .. goff[g + 1] and a
// threshold t_g = coff[g + 1] - coff[g], the number of its Feldman commitments.
//   tc_candidate         a partial signature that can be interpolated at all: decodes, on the curve, not the identity
//   tc_repeats           the share's id (its 32 bytes) occurs EARLIER in its group: of several equal ids every one but the
//                        first reports it, which is enough to mark the group
//   tc_rank              the share's place among the set bits of its group in a bitmap over the call's shares (LSB-first, as
//                        every bitmap of the ABI), and the group's number of set bits
//   tc_pick              the first t_g set shares of a group that has at least t_g of them and carries no mark are the ones
//                        interpolated: share -> slot coff[g] + rank of the compacted arrays, which therefore hold exactly t_g
//                        slots per group and are described by the coefficient offsets
// Selection only: no field arithmetic beyond the curve equation of tc_candidate, no data-dependent heavy branch.
// tests/hostsim/threshold_checked_host.cpp runs the same functions on the host with -DBN_CHECK against a Python model.  They
// are not a CPU fallback: nothing in the product's host path calls them.
#pragma once
#include "threshold_deal.h"

namespace bn {

constexpr uint32_t TC_MARK_SHORT = 4u;           // gstat bit (beside TD_MARK_SCALAR / TD_MARK_POINT): t_g == 0 or fewer than t_g set shares

BN_INL bool tc_bit(const uint8_t* bm, size_t i) { return (bm[i >> 3] >> (i & 7)) & 1u; }
// bit i of a AND b; b == null stands for all ones
BN_INL bool tc_set(const uint8_t* a, const uint8_t* b, size_t i) { return tc_bit(a, i) & (b ? tc_bit(b, i) : true); }

BN_INL bool tc_candidate(const uint8_t* sig) {
  bool ok;
  const G1A p = th_point(sig, ok);
  return ok & !p.inf;
}

// word k (0 .. 7) of id i, assembled from bytes: the ids need no alignment
BN_INL uint32_t tc_id_word(const uint8_t* ids, size_t i, int k) {
  const uint8_t* p = ids + 32 * i + 4 * k;
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
// ids: the call's ids; a: the first share of the group of share s
BN_INL bool tc_repeats(const uint8_t* ids, uint32_t a, uint32_t s) {
  uint32_t me[8];
  for (int k = 0; k < 8; ++k) me[k] = tc_id_word(ids, s, k);
  bool rep = false;
#pragma unroll 1
  for (uint32_t j = a; j < s; ++j) {
    uint32_t d = 0;
    for (int k = 0; k < 8; ++k) d |= me[k] ^ tc_id_word(ids, j, k);
    rep |= d == 0;
  }
  return rep;
}

struct TcRank { bool set; uint32_t rank, total; };
// share s of the group [a, b) in the bitmap bits_a AND bits_b over the call's shares
BN_INL TcRank tc_rank(const uint8_t* bits_a, const uint8_t* bits_b, uint32_t a, uint32_t b, uint32_t s) {
  TcRank r{tc_set(bits_a, bits_b, s), 0, 0};
#pragma unroll 1
  for (uint32_t j = a; j < b; ++j) {
    const uint32_t v = tc_set(bits_a, bits_b, j) ? 1u : 0u;
    r.total += v;
    r.rank += j < s ? v : 0u;
  }
  return r;
}
// a group without a threshold, or with fewer set shares than its threshold, cannot be interpolated
BN_INL bool tc_short(const TcRank& r, uint32_t t) { return (t == 0) | (r.total < t); }
// marks: the group's mark word as the id and commitment checks left it (TC_MARK_SHORT is not looked at: the lane knows)
BN_INL bool tc_pick(const TcRank& r, uint32_t t, uint32_t marks) {
  return r.set & (r.rank < t) & !tc_short(r, t) & ((marks & (TD_MARK_SCALAR | TD_MARK_POINT)) == 0);
}

}  // namespace bn
