// keyset_committee_merge.h -- what ONE lane does in the checked merge of partial aggregates PER COMMITTEE of a registered key
// set (k_keyset_committee_merge.hip, host_keyset_committee_merge.hip).  A call brings N CONTRIBUTIONS (a row as
// wide as the group's committee, bit j = member j of the committee is in it, and a 64-byte aggregate signature) in n_groups
// ragged groups, group g naming committee com[g] and owning the contributions goff[g] .. goff[g + 1], one message per group.
// Everything keyset_merge.h does per 32-key word of the REGISTRY is done here per 32-member word of a COMMITTEE, with the
// functions of keyset_merge.h themselves: a committee's row is a registry row whose "keys" are the positions, and the
// committee's validity words (keyset_committee.h cvalid) are its KeyValidate words.  What is new is where a group's rows lie:
//   kcm_group       the view of group g that km_test / km_flags / km_take / km_begin / km_end take: the width of its rows from
//                   the committee record (KcCom: size), its validity words at the committee's word base, its contribution rows
//                   back to back from the byte offset rbase[g], its merged row at the byte offset roff[g]
//   kcm_row         contribution s of that group
// No member index is gathered and no registry-wide word is read.  keyset_committee_merge_plan.h (included here) is the plain C++
// of the host side.  tests/hostsim/keyset_committee_merge_host.cpp compiles both for the host with -DBN_CHECK, runs a wave as 64
// lane states in lockstep and forms the votes itself.  The lane functions are not a CPU fallback: nothing in the product's host
// path calls them.
#pragma once
#include "keyset_merge.h"
#include "keyset_committee.h"
#include "keyset_committee_merge_plan.h"

namespace bn {

// rows: the group's contribution rows (contribution a first); valid: the committee's validity words; urow: the merged row;
// rb / W: the bytes / words of every row of the group; a .. b: the group's contributions
struct KcmGroup { const uint8_t* rows; const uint32_t* valid; uint8_t* urow; uint32_t rb, W, a, b; };
// k_size / k_wbase: the size and the word base of the group's committee (KcCom); goff: the groups' contribution offsets
BN_INL KcmGroup kcm_group(uint32_t k_size, uint32_t k_wbase, const uint32_t* cvalid, const uint32_t* goff, const uint64_t* rbase, const uint64_t* roff, size_t g,
                          const uint8_t* rows, uint8_t* urows) {
  KcmGroup v;
  v.rb = ks_row_bytes(k_size); v.W = ks_words(k_size);
  v.valid = cvalid + k_wbase;
  v.rows = rows + rbase[g];
  v.urow = urows + roff[g];
  v.a = goff[g]; v.b = goff[g + 1];
  return v;
}
BN_INL const uint8_t* kcm_row(const KcmGroup& v, uint32_t s) { return v.rows + (size_t)(s - v.a) * v.rb; }

}  // namespace bn
