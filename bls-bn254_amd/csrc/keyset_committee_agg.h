// keyset_committee_agg.h -- what ONE lane does in the checked signature aggregation per COMMITTEE of a registered key set
// (k_keyset_committee_agg.hip, host_keyset_committee_agg.hip).  A call brings N ENTRIES (position in the member
// list of the group's committee, 64-byte signature) in n_groups ragged groups, group g naming committee com[g] and owning the
// entries goff[g] .. goff[g + 1] with strictly increasing positions, one message per group.  Everything keyset_agg.h does per key
// index of the REGISTRY is done here per position of a COMMITTEE, with the functions of keyset_agg.h themselves where they fit:
//   kca_group       the group of an entry: the last g with goff[g] <= s, by binary search (empty groups own no entry and are
//                   stepped over); kca_word_group: the same over the 64-bit prefix of the groups' row words
//   kca_scan        ka_scan with the key's validity read from the COMMITTEE's validity words (keyset_committee.h cvalid): the bit
//                   of the entry's position, so no member index is gathered
//   kca_resolve     the fallback only: the registry index of an entry, members[first member + position]
// The rows are ka_row_word / ka_row_store of keyset_agg.h on positions: a committee's row is a registry row whose "keys" are the
// positions.  A lane reads its group's inputs and the bitmap of an EARLIER launch, never another lane's result of its own
// launch, so a launch may end anywhere.  keyset_committee_agg_plan.h (included here) is the plain C++ of the host side.
// tests/hostsim/keyset_committee_aggregate_host.cpp compiles both for the host with -DBN_CHECK against a Python model.  The lane
// functions are not a CPU fallback: nothing in the product's host path calls them.
#pragma once
#include "keyset_agg.h"
#include "keyset_committee.h"
#include "keyset_committee_agg_plan.h"

namespace bn {

// goff[0 .. n_groups] non-decreasing, goff[0] = 0, s < goff[n_groups]: the g with goff[g] <= s < goff[g + 1]
BN_INL uint32_t kca_group(const uint32_t* goff, uint32_t n_groups, uint32_t s) {
  uint32_t a = 0, b = n_groups;
  while (a < b) {
    const uint32_t mid = a + ((b - a) >> 1);
    if (goff[mid + 1] <= s) a = mid + 1; else b = mid;
  }
  return a;
}
BN_INL uint32_t kca_word_group(const uint64_t* wpre, uint32_t n_groups, uint64_t t) {
  uint32_t a = 0, b = n_groups;
  while (a < b) {
    const uint32_t mid = a + ((b - a) >> 1);
    if (wpre[mid + 1] <= t) a = mid + 1; else b = mid;
  }
  return a;
}
// entry s of the call, in a group of the committee whose validity words are cvalid (at its word base): pos / sigs = the call's
// entries, mask = a bitmap over the call's entries or null (all ones)
BN_FUNC KaScan kca_scan(const uint32_t* cvalid, const uint32_t* pos, const uint8_t* sigs, const uint8_t* mask, size_t s) {
  BN_CTX;
  bool ok;
  const G1A a = th_point(sigs + 64 * s, ok);             // the stand-in (1, 2) where it does not decode or is off the curve
  KaScan r;
  r.cand = ok & !a.inf & (kc_bit(cvalid, pos[s]) != 0) & (mask ? tc_bit(mask, s) : true);
  r.p = proj_select(r.cand, proj_from_affine(a), proj_identity<Fp>());
  return r;
}
// kca_scan for 32-byte entries, as ka_scan_wire is ka_scan for them (keyset_agg.h)
BN_FUNC KaScan kca_scan_wire(const uint32_t* cvalid, const uint32_t* pos, const uint8_t* sigs, const uint8_t* mask, size_t s) {
  BN_CTX;
  bool ok;
  const G1A a = g1_inflate_point(sigs + 32 * s, ok);     // the stand-in (1, 2) where it does not inflate
  KaScan r;
  r.cand = ok & !a.inf & (kc_bit(cvalid, pos[s]) != 0) & (mask ? tc_bit(mask, s) : true);
  r.p = proj_select(r.cand, proj_from_affine(a), proj_identity<Fp>());
  return r;
}
// members: the committee's (at its first member)
BN_INL uint32_t kca_resolve(const uint32_t* members, const uint32_t* pos, size_t s) { return members[pos[s]]; }

}  // namespace bn
