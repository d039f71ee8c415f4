// keyset_committee_plan.h -- the host side of the committees over a registered key set that needs neither HIP nor the context
// (host_keyset_committee.hip; the lane functions are in keyset_committee.h): the check of a committee table, the argument walk of
// a call over ragged groups, and the plan of its sums.  Plain C++ over the standard library only, beside keyset_agg_plan.h, so
// that tests/hostsim/keyset_committee_host.cpp compiles it for the CPU.  See DESIGN.md 6l.
//
// A committee is a list of key indices; a group names a committee and brings a row as wide as that committee, so groups are
// RAGGED: committee c has words(c) = ceil(size_c / 32) words.  The plan of a call:
//   order[]      a stable counting sort of the groups by committee: sorted position -> caller's group.  Groups of one committee
//                become neighbours, so one staged word of a committee serves many of them
//   per sorted group   its committee, the byte offset of its row, and the base of its word partials inside its launch
//   items        {committee word (global index), member base, first sorted position, count}: ONE word of ONE committee across up
//                to KC_ITEM_GROUPS consecutive sorted groups of that committee; one workgroup of the word kernel each
//   launches     cut at sorted-group boundaries so that a launch's partials stay within `part_max` and its groups within
//                `chunk` (a group whose committee alone has more words than part_max is a launch of its own)
//   reduction    the partials of a launch are GROUP-major -- group i owns [pbase_i, pbase_i + words_i) -- which is the contiguous
//                segment layout plan_seg_levels (seg_plan.h) cuts into runs of KC_RUN: the levels are its, not a private loop
#pragma once
#include <string>
#include "seg_plan.h"

constexpr size_t KC_ITEM_GROUPS = 64;            // groups of one item: one wave (keyset_committee.h KC_LANES)
constexpr size_t KC_RUN = 16;                    // partials per lane of a reduction level (k_g2_seg_sum)
constexpr size_t KC_MAX_COMMITTEES = (size_t)1 << 16;
constexpr size_t KC_MAX_MEMBERS = (size_t)1 << 22;   // the default launch chunk (BLSBN254_CHUNK_LANES)
constexpr size_t KC_LAUNCH_PARTIALS = (size_t)1 << 20;   // host_keyset.hip KS_LAUNCH_ITEMS (a static_assert there keeps them equal)

// one committee as the device reads it (16 bytes): its first member, its size, the base of its words
struct KcCom { uint32_t off, size, wbase, pad; };
// the host mirror of a table: the committees, the committee of every committee word, the member and word counts
struct KcTable {
  std::vector<KcCom> com;
  std::vector<uint32_t> wcom;
  size_t members = 0, words = 0;
  void clear() { com.clear(); wcom.clear(); members = words = 0; }
};
static inline uint32_t kc_words(uint32_t size) { return (size + 31) / 32; }
static inline uint32_t kc_row_bytes(uint32_t size) { return (size + 7) / 8; }

// The checks of blsbn254_keyset_set_committees and the table they pass.  false: err names the committee.
static inline bool kc_build_table(const uint32_t* members, const uint64_t* com_off, size_t n_com, size_t n_keys, KcTable& t, std::string& err) {
  t.clear();
  if (n_com == 0 || n_com > KC_MAX_COMMITTEES) { err = "1 to 65536 committees"; return false; }
  if (com_off[0] != 0) { err = "committee 0: the offsets do not start at 0"; return false; }
  t.com.resize(n_com);
  for (size_t c = 0; c < n_com; ++c) {
    const std::string who = "committee " + std::to_string(c);
    if (com_off[c + 1] < com_off[c]) { t.clear(); err = who + ": the offsets decrease"; return false; }
    if (com_off[c + 1] == com_off[c]) { t.clear(); err = who + " is empty"; return false; }
    if (com_off[c + 1] > KC_MAX_MEMBERS) { t.clear(); err = who + ": more than 4194304 members in the table"; return false; }
    const uint32_t size = (uint32_t)(com_off[c + 1] - com_off[c]);
    t.com[c] = {(uint32_t)com_off[c], size, (uint32_t)t.words, 0};
    t.words += kc_words(size);
  }
  t.members = (size_t)com_off[n_com];
  std::vector<uint32_t> seen(n_keys, 0);                       // the last committee + 1 that listed the key
  t.wcom.reserve(t.words);
  for (size_t c = 0; c < n_com; ++c) {
    const KcCom& k = t.com[c];
    for (uint32_t j = 0; j < k.size; ++j) {
      const uint32_t key = members[k.off + j];
      const auto who = [c] { return "committee " + std::to_string(c); };
      if (key >= n_keys) { t.clear(); err = who() + ": member " + std::to_string(j) + " names key " + std::to_string(key) + " of " + std::to_string(n_keys); return false; }
      if (seen[key] == c + 1) { t.clear(); err = who() + " lists key " + std::to_string(key) + " twice"; return false; }
      seen[key] = (uint32_t)c + 1;
    }
    t.wcom.insert(t.wcom.end(), kc_words(k.size), (uint32_t)c);
  }
  return true;
}

// The argument walk of a call over rows: com[g] names a committee, row g = sel[sel_off[g] .. sel_off[g + 1]) is exactly as wide
// as it, and sets no bit past its last member.  false: err names the group.
static inline bool kc_check_rows(const KcTable& t, const uint32_t* com, const uint8_t* sel, const uint64_t* sel_off, size_t n_groups, std::string& err) {
  for (size_t g = 0; g < n_groups; ++g) {
    const std::string who = "group " + std::to_string(g);
    if (com[g] >= t.com.size()) { err = who + " names committee " + std::to_string(com[g]) + " of " + std::to_string(t.com.size()); return false; }
    const uint32_t size = t.com[com[g]].size, rb = kc_row_bytes(size);
    if (sel_off[g + 1] < sel_off[g] || sel_off[g + 1] - sel_off[g] != rb) { err = who + ": the row must be " + std::to_string(rb) + " bytes"; return false; }
    if ((size & 7) && (sel[sel_off[g + 1] - 1] & (uint8_t)(0xffu << (size & 7)))) { err = who + ": the row sets a bit past the last member"; return false; }
  }
  return true;
}

struct KcItem { uint32_t cword, mbase, first, count; };
// sorted groups [lo, hi), their items [item0, item0 + n_items), the partials they write and the levels that reduce them
struct KcLaunch { size_t lo, hi, item0, n_items, partials; std::vector<SegLevel> levels; };
struct KcPlan {
  std::vector<uint32_t> order, scom, spbase;     // per sorted position: caller's group, committee, partial base in its launch
  std::vector<uint64_t> srow;                    // ... and the byte offset of its row behind sel_off[0]
  std::vector<KcItem> items;
  std::vector<KcLaunch> launches;
  size_t items_max = 1, partials_max = 1;        // the largest level between the first and the last; the largest launch
};
// the partials one launch may hold under a launch chunk
static inline size_t kc_part_max(size_t chunk) { return std::min(KC_LAUNCH_PARTIALS, chunk); }

// The plan of a call whose arguments passed kc_check_rows.  The descriptors of the reduction levels are appended to start / len
// (cleared first).  false: the levels do not converge (cannot happen).
static inline bool kc_plan(const KcTable& t, const uint32_t* com, const uint64_t* sel_off, size_t n_groups, size_t chunk, KcPlan& p,
                           std::vector<uint32_t>& start, std::vector<uint32_t>& len) {
  const size_t n_com = t.com.size(), part_max = kc_part_max(chunk);
  p.order.resize(n_groups); p.scom.resize(n_groups); p.spbase.resize(n_groups); p.srow.resize(n_groups);
  p.items.clear(); p.launches.clear(); p.items_max = p.partials_max = 1;
  start.clear(); len.clear();
  // the stable counting sort
  std::vector<size_t> at(n_com + 1, 0);
  for (size_t g = 0; g < n_groups; ++g) ++at[com[g] + 1];
  for (size_t c = 0; c < n_com; ++c) at[c + 1] += at[c];
  for (size_t g = 0; g < n_groups; ++g) p.order[at[com[g]]++] = (uint32_t)g;
  for (size_t i = 0; i < n_groups; ++i) {
    const size_t g = p.order[i];
    p.scom[i] = com[g]; p.srow[i] = sel_off[g] - sel_off[0];
  }
  for (size_t lo = 0; lo < n_groups;) {
    KcLaunch L;
    L.lo = lo; L.item0 = p.items.size(); L.partials = 0;
    size_t hi = lo;
    std::vector<SegRange> seg;
    while (hi < n_groups && hi - lo < chunk) {
      const size_t w = kc_words(t.com[p.scom[hi]].size);
      if (hi > lo && L.partials + w > part_max) break;
      p.spbase[hi] = (uint32_t)L.partials;
      seg.push_back({L.partials, L.partials + w});
      L.partials += w; ++hi;
    }
    L.hi = hi;
    // runs of one committee, cut into items of at most KC_ITEM_GROUPS groups, one item per word
    for (size_t a = lo; a < hi;) {
      const KcCom& k = t.com[p.scom[a]];
      size_t b = a;
      while (b < hi && p.scom[b] == p.scom[a]) ++b;
      for (size_t f = a; f < b; f += KC_ITEM_GROUPS)
        for (uint32_t w = 0; w < kc_words(k.size); ++w)
          p.items.push_back({k.wbase + w, k.off + 32 * w, (uint32_t)f, (uint32_t)std::min(KC_ITEM_GROUPS, b - f)});
      a = b;
    }
    L.n_items = p.items.size() - L.item0;
    if (!plan_seg_levels(seg, KC_RUN, start, len, L.levels, &p.items_max)) return false;
    p.partials_max = std::max(p.partials_max, L.partials);
    p.launches.push_back(std::move(L));
    lo = hi;
  }
  return true;
}
