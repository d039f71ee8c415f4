// keyset_merge.h -- what ONE lane does in the checked merge of partial aggregates over a REGISTERED key set (k_keyset_merge.hip,
// host_keyset_merge.hip).  A call brings N CONTRIBUTIONS (a row of ceil(n_keys / 8) bytes, bit i = key i is in it, and a 64-byte
// aggregate signature) in n_groups ragged groups, group g owning the contributions off[g] .. off[g + 1], one message per group.
//   km_sig          one lane per contribution: tc_candidate of the signature as a byte, and the signature as a projective point
//                   for the segmented G1 sum (the identity where it fails the test)
//   km_test         one lane of the WAVE that walks a group, lane l owning the 32-key words l, l + 64, ... of every row: the
//                   lane's share of the three votes on a contribution -- some bit set, a bit on a key without the KeyValidate
//                   bit, a bit that the union of the rows selected so far already has.  The wave ORs the shares (__any)
//   km_flags        the contribution's byte from the votes: KM_CAND (the signature passes, the row is not empty and selects valid
//                   keys only) and KM_USED (a candidate, its mask bit set, disjoint from the union)
//   km_take         a used contribution's words ORed into the lane's words of the union
//   km_begin / km_end   the union of a group: ONE register per lane while the row has at most 64 words (stored as the group's
//                   merged row at the end), the group's merged row itself above that (cleared first; a lane reads back only
//                   the words it wrote)
//   km_drop_point   one lane per contribution: the identity over the point of a contribution that is not used, so that the
//                   segmented sum needs no compaction
// A lane reads and writes its OWN words of the union only: the votes are the only traffic between lanes.  Rows are byte arrays
// whose length is in general no multiple of 4: they are read as ka_row_store writes them, byte by byte into words
// (ks_row_word), four consecutive bytes per lane and 256 consecutive bytes per wave and trip.
// keyset_merge_plan.h (included here) is the plain C++ of the host side.  tests/hostsim/keyset_merge_host.cpp compiles both for
// the host with -DBN_CHECK, runs a wave as 64 lane states in lockstep and forms the votes itself.  The lane functions are not a
// CPU fallback: nothing in the product's host path calls them.
#pragma once
#include "keyset_agg.h"
#include "keyset_merge_plan.h"

namespace bn {

constexpr uint32_t KM_WAVE = 64;                 // lanes that share a group; the stride of a lane's words
constexpr uint8_t KM_USED = 1, KM_CAND = 2;      // bits of a contribution's byte

struct KmSig { bool ok; G1P p; };
BN_FUNC KmSig km_sig(const uint8_t* sigs, size_t s) {
  BN_CTX;
  bool ok;
  const G1A a = th_point(sigs + 64 * s, ok);             // the stand-in (1, 2) where it does not decode or is off the curve
  KmSig r;
  r.ok = ok & !a.inf;
  r.p = proj_select(r.ok, proj_from_affine(a), proj_identity<Fp>());
  return r;
}
BN_FUNC void km_drop_point(int32_t* ws, size_t stride) {
  BN_CTX;
  ka_store_point(ws, stride, proj_identity<Fp>());
}

struct KmVote { bool some, invalid, overlap; };
// row: the contribution's; valid: the key set's KeyValidate bits, a word per 32 keys; the union: ureg while W <= KM_WAVE (the
// lane's one word), else the lane's words of urow
BN_INL KmVote km_test(const uint8_t* row, uint32_t row_bytes, uint32_t W, uint32_t lane, const uint32_t* valid, const uint8_t* urow, uint32_t ureg) {
  KmVote v{false, false, false};
#pragma unroll 1
  for (uint32_t w = lane; w < W; w += KM_WAVE) {
    const uint32_t x = ks_row_word(row, row_bytes, w);
    const uint32_t u = W <= KM_WAVE ? ureg : ks_row_word(urow, row_bytes, w);
    v.some |= x != 0;
    v.invalid |= (x & ~valid[w]) != 0;
    v.overlap |= (x & u) != 0;
  }
  return v;
}
// any: the three votes of the wave
BN_INL uint8_t km_flags(bool sig_ok, bool mask_bit, const KmVote& any) {
  const bool cand = sig_ok & any.some & !any.invalid;
  return (uint8_t)((cand ? KM_CAND : 0) | ((cand & mask_bit & !any.overlap) ? KM_USED : 0));
}
BN_INL void km_take(const uint8_t* row, uint32_t row_bytes, uint32_t W, uint32_t lane, uint8_t* urow, uint32_t& ureg) {
#pragma unroll 1
  for (uint32_t w = lane; w < W; w += KM_WAVE) {
    const uint32_t x = ks_row_word(row, row_bytes, w);
    if (W <= KM_WAVE) ureg |= x;
    else ka_row_store(urow, row_bytes, w, ks_row_word(urow, row_bytes, w) | x);
  }
}
BN_INL void km_begin(uint8_t* urow, uint32_t row_bytes, uint32_t W, uint32_t lane, uint32_t& ureg) {
  ureg = 0;
  if (W <= KM_WAVE) return;
#pragma unroll 1
  for (uint32_t w = lane; w < W; w += KM_WAVE) ka_row_store(urow, row_bytes, w, 0);
}
BN_INL void km_end(uint8_t* urow, uint32_t row_bytes, uint32_t W, uint32_t lane, uint32_t ureg) {
  if (W <= KM_WAVE && lane < W) ka_row_store(urow, row_bytes, lane, ureg);
}

}  // namespace bn
