// keyset_committee_agg_plan.h -- the host side of the checked signature aggregation per COMMITTEE of a registered key set that
// needs neither HIP nor the context (host_keyset_committee_agg.hip; the lane functions are in keyset_committee_agg.h): the walk
// over a call's committees, positions and offsets, the ragged layout of its rows, and the repack of the groups that go to the
// per-signature fallback.  Plain C++ over the standard library only, beside keyset_agg_plan.h and keyset_committee_plan.h, so that
// tests/hostsim/keyset_committee_aggregate_host.cpp compiles it for the CPU.  See DESIGN.md 6o.
//
// A group names a committee (keyset_committee_plan.h KcTable) and brings entries (position in the committee's member list,
// signature) with strictly increasing positions; its row is as wide as its committee, ceil(size / 8) bytes at the byte offset the
// caller's sel_off gives it, so rows are RAGGED and in general neither aligned nor a multiple of 4 bytes long.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "keyset_committee_plan.h"

// The walk over the call's arguments: KCA_OK, or the first thing that is wrong and where.  pos is indexed by the entry offsets
// themselves (which need not start at 0), com by the group; max_entries bounds sig_off[n_groups] - sig_off[0].  Order: the entry
// offsets of every group, the entry count, then group by group its committee, its row length and its positions.
enum KcaWalkCode { KCA_OK = 0, KCA_OFF_DECREASE, KCA_TOO_MANY, KCA_COM_RANGE, KCA_ROW_LEN, KCA_POS_RANGE, KCA_POS_ORDER };
struct KcaWalk { KcaWalkCode code; size_t group; uint64_t entry; };
static inline KcaWalk kca_walk(const KcTable& t, const uint32_t* com, const uint32_t* pos, const uint64_t* sig_off, const uint64_t* sel_off, size_t n_groups,
                               uint64_t max_entries) {
  for (size_t g = 0; g < n_groups; ++g)
    if (sig_off[g + 1] < sig_off[g]) return {KCA_OFF_DECREASE, g, sig_off[g]};
  if (sig_off[n_groups] - sig_off[0] > max_entries) return {KCA_TOO_MANY, 0, 0};
  for (size_t g = 0; g < n_groups; ++g) {
    if (com[g] >= t.com.size()) return {KCA_COM_RANGE, g, sig_off[g]};
    const uint32_t size = t.com[com[g]].size;
    if (sel_off[g + 1] < sel_off[g] || sel_off[g + 1] - sel_off[g] != kc_row_bytes(size)) return {KCA_ROW_LEN, g, sig_off[g]};
    for (uint64_t s = sig_off[g]; s < sig_off[g + 1]; ++s) {
      if (pos[s] >= size) return {KCA_POS_RANGE, g, s};
      if (s > sig_off[g] && pos[s] <= pos[s - 1]) return {KCA_POS_ORDER, g, s};
    }
  }
  return {KCA_OK, 0, 0};
}

// The ragged layout of a call that passed the walk: wpre[g] = the 32-member words of the groups before g (wpre[n_groups] = the
// lanes of the rows kernel), roff[g] = the byte offset of row g behind sel_off[0].
static inline void kca_layout(const KcTable& t, const uint32_t* com, const uint64_t* sel_off, size_t n_groups, std::vector<uint64_t>& wpre,
                              std::vector<uint64_t>& roff) {
  wpre.assign(n_groups + 1, 0); roff.assign(n_groups + 1, 0);
  for (size_t g = 0; g < n_groups; ++g) {
    wpre[g + 1] = wpre[g] + kc_words(t.com[com[g]].size);
    roff[g + 1] = sel_off[g + 1] - sel_off[0];
  }
}

// The sub-call of the groups in `fail` (ascending group numbers of the call): of each group the CANDIDATE entries only, which are
// the entries whose position's bit is set in the group's row (positions do not repeat inside a group).  rows: the call's rows
// as downloaded, row g at rows + (sel_off[g] - sel_off[0]).  com / pos: the sub-call's committees and positions; src: the call
// position (an index into the caller's pos / sigs) each entry came from; off / sel_off: the sub-call's offsets, from 0.
struct KcaRepack { std::vector<uint32_t> com, pos; std::vector<uint64_t> src, off, sel_off; };
static inline void kca_repack(const std::vector<size_t>& fail, const uint32_t* com, const uint32_t* pos, const uint64_t* sig_off, const uint64_t* sel_off,
                              const uint8_t* rows, KcaRepack& out) {
  out.com.clear(); out.pos.clear(); out.src.clear(); out.off.assign(1, 0); out.sel_off.assign(1, 0);
  for (size_t g : fail) {
    const uint8_t* row = rows + (sel_off[g] - sel_off[0]);
    for (uint64_t s = sig_off[g]; s < sig_off[g + 1]; ++s)
      if ((row[pos[s] >> 3] >> (pos[s] & 7)) & 1) { out.pos.push_back(pos[s]); out.src.push_back(s); }
    out.com.push_back(com[g]);
    out.off.push_back(out.pos.size());
    out.sel_off.push_back(out.sel_off.back() + (sel_off[g + 1] - sel_off[g]));
  }
}
