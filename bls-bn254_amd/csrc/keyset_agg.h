// keyset_agg.h -- what ONE lane does in the checked signature aggregation over a REGISTERED key set (k_keyset_agg.hip,
// host_keyset_agg.hip).  A call brings N ENTRIES (key index, 64-byte signature) in n_groups
// ragged groups, group g owning the entries off[g] .. off[g + 1] with strictly increasing key indices, one message per group.
//   ka_scan         one lane per entry: the candidate bit (the key's KeyValidate byte, tc_candidate of the signature, and the
//                   bit of an optional mask bitmap over the call's entries) and the signature as a projective point for the
//                   segmented G1 sum, the identity for a non-candidate
//   ka_scan_wire    the same for 32-byte entries (g1_inflate_point of inflate.h); ka_wire_out: a group's sum in both encodings
//   ka_row_word     one lane per (group, 32-key word): the word of the group's participation row, found by binary search in
//                   the group's sorted indices and ORed from the candidate bits of the entries that fall into the word
//   ka_row_store    the word's bytes into a row of ceil(n_keys / 8) bytes (rows need no alignment: bytes, not words)
// Selection only: no field arithmetic beyond the curve equation of the candidate test.  A lane reads its group's inputs and the
// bitmap of an EARLIER launch, never another lane's result of its own launch, so a launch may end anywhere.
// keyset_agg_plan.h (included here) is the plain C++ of the host side: the argument walk and the repack of the groups that go
// to the fallback.  tests/hostsim/keyset_aggregate_host.cpp compiles both for the host with -DBN_CHECK against a Python model.
// The lane functions are not a CPU fallback: nothing in the product's host path calls them.
#pragma once
#include "threshold_checked.h"
#include "inflate.h"
#include "keyset.h"
#include "keyset_agg_plan.h"

namespace bn {

struct KaScan { bool cand; G1P p; };
// entry s of the call: key_valid = the key set's KeyValidate bytes, idx / sigs = the call's entries, mask = a bitmap over the
// call's entries or null (all ones)
BN_FUNC KaScan ka_scan(const uint8_t* key_valid, const uint32_t* idx, const uint8_t* sigs, const uint8_t* mask, size_t s) {
  BN_CTX;
  bool ok;
  const G1A a = th_point(sigs + 64 * s, ok);             // the stand-in (1, 2) where it does not decode or is off the curve
  KaScan r;
  r.cand = ok & !a.inf & (key_valid[idx[s]] != 0) & (mask ? tc_bit(mask, s) : true);
  r.p = proj_select(r.cand, proj_from_affine(a), proj_identity<Fp>());
  return r;
}
// ka_scan for entries that arrive in wire format: sigs holds 32 bytes per entry, the point comes from
// g1_inflate_point, whose square test of the root is the curve test th_point runs.  The candidate bit and the point are those of
// ka_scan on g1_inflate's bytes: an entry that does not inflate is the marker there and no candidate here.
BN_FUNC KaScan ka_scan_wire(const uint8_t* key_valid, const uint32_t* idx, const uint8_t* sigs, const uint8_t* mask, size_t s) {
  BN_CTX;
  bool ok;
  const G1A a = g1_inflate_point(sigs + 32 * s, ok);     // the stand-in (1, 2) where it does not inflate
  KaScan r;
  r.cand = ok & !a.inf & (key_valid[idx[s]] != 0) & (mask ? tc_bit(mask, s) : true);
  r.p = proj_select(r.cand, proj_from_affine(a), proj_identity<Fp>());
  return r;
}
// the layout k_g1_seg_sum reads: x, y, z limb-major
BN_FUNC void ka_store_point(int32_t* ws, size_t stride, const G1P& p) {
  store_fp(ws, stride, p.x); store_fp(ws + NL * stride, stride, p.y); store_fp(ws + 2 * NL * stride, stride, p.z);
}
BN_FUNC G1P ka_load_point(const int32_t* ws, size_t stride) {
  return {load_fp(ws, stride), load_fp(ws + NL * stride, stride), load_fp(ws + 2 * NL * stride, stride)};
}
// A group's sum in both encodings from ONE conversion to affine and one pass out of Montgomery form per coordinate: full = the 64
// bytes g1_encode writes (what the verify pipeline reads), wire = the 32 bytes g1_compress writes (what the caller gets), the
// parity of the canonical y as the flag; the identity is (0, 1) in both.
BN_FUNC void ka_wire_out(const G1P& p, uint8_t* full, uint8_t* wire) {
  BN_CTX;
  const G1A a = g1_to_affine(p);
  const Fp x = fp_from_mont(fp_select(a.inf, fp_zero(), a.x)), y = fp_from_mont(fp_select(a.inf, fp_one(), a.y));
  uint32_t wx[8], wy[8];
  limbs_to_words(wx, x.l); limbs_to_words(wy, y.l);
  BN_UNROLL for (int j = 0; j < 8; ++j) {
    store_be32(full + 4 * (7 - j), wx[j]); store_be32(full + 32 + 4 * (7 - j), wy[j]);
    store_be32(wire + 4 * (7 - j), j == 7 ? wx[j] | ((wy[0] & 1u) << 31) : wx[j]);
  }
}

// the first s in [a, b) with idx[s] >= key (b if none); idx strictly increasing over [a, b)
BN_INL uint32_t ka_lower(const uint32_t* idx, uint32_t a, uint32_t b, uint32_t key) {
  while (a < b) {
    const uint32_t mid = a + ((b - a) >> 1);
    if (idx[mid] < key) a = mid + 1; else b = mid;
  }
  return a;
}
// word w of the row of the group [a, b): bit (idx[s] - 32 w) for every candidate entry s whose key lies in the word
BN_INL uint32_t ka_row_word(const uint32_t* idx, const uint8_t* cand, uint32_t a, uint32_t b, uint32_t w) {
  uint32_t v = 0;
  const uint32_t s0 = ka_lower(idx, a, b, 32 * w);
#pragma unroll 1
  for (uint32_t s = s0; s < b; ++s) {
    const uint32_t k = idx[s] - 32 * w;
    if (k >= 32) break;
    v |= (tc_bit(cand, s) ? 1u : 0u) << k;
  }
  return v;
}
BN_INL void ka_row_store(uint8_t* row, uint32_t row_bytes, uint32_t w, uint32_t v) {
  for (uint32_t k = 0; k < 4; ++k)
    if (4 * w + k < row_bytes) row[4 * w + k] = (uint8_t)(v >> (8 * k));
}

}  // namespace bn

