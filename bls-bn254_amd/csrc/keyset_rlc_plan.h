// keyset_rlc_plan.h -- the host side of the key-set FastAggregateVerify by random linear combination per message that needs
// neither HIP nor the context (host_keyset_rlc.hip; the lane functions are in keyset_rlc.h): which groups of a call share a
// message, the order that makes them neighbours, the chunks one pairing equation decides, and the runs of the two segmented
// sums that reduce a chunk.  Plain C++ over the standard library only, beside seg_plan.h, so that
// tests/hostsim/keyset_rlc_host.cpp compiles it for the CPU.  See DESIGN.md 6m.
//
//   classes      the groups whose messages are byte-identical (a hash map over the bytes, full comparison), numbered in the order
//                of their first appearance
//   order[]      a stable counting sort of the groups by class: sorted position -> caller's group; pos[] is its inverse
//   chunks       a class's run of sorted positions cut into pieces of at most C groups: {start, len, class}.  Eligibility is only
//                known on the device, so chunks are cut over ALL groups of a class; an ineligible member contributes the identity
//   reduction    the weighted points are written at their SORTED positions, so a chunk is a contiguous segment: the levels are
//                those of plan_seg_levels (seg_plan.h) in runs of KSR_RUN, one launch for the call
#pragma once
#include <string_view>
#include <unordered_map>
#include "seg_plan.h"

constexpr size_t KSR_DEFAULT_GROUP = 64;         // groups per chunk unless blsbn254_set_keyset_rlc_group says otherwise
constexpr size_t KSR_MIN_GROUP = 2, KSR_MAX_GROUP = 4096;
constexpr size_t KSR_RUN = 16;                   // points per lane of a reduction level (k_g1_seg_sum, k_g2_seg_sum)

// what becomes of a chunk once its sums are known: too few eligible members to gain anything (they go to the exact list), one
// pairing equation, or a weighted sum that is the identity (to the exact list as well)
enum : uint8_t { KSR_DIRECT = 0, KSR_CHECK = 1, KSR_DEGENERATE = 2 };

struct KsrChunk { uint32_t start, len, cls; };   // sorted positions [start, start + len) of class cls
struct KsrPlan {
  std::vector<uint32_t> order, pos;              // sorted position -> caller's group, and back
  std::vector<uint32_t> chunk_of;                // per caller's group: its chunk
  std::vector<uint32_t> rep;                     // per class: the first group that brought its message
  std::vector<uint8_t> multi;                    // per caller's group: its chunk has at least two members
  std::vector<KsrChunk> chunks;
  std::vector<SegLevel> levels;                  // of the segmented sums over the chunks
  size_t items_max = 1;                          // the largest level between the first and the last
  size_t n_multi = 0;                            // groups in chunks of at least two
};

// The plan of a call of n_groups > 0 groups with messages msgs[off[g] .. off[g + 1]) (offsets checked by the caller) at C groups
// per chunk.  The descriptors of the reduction levels are appended to start / len (cleared first).  false: the levels do not
// converge (cannot happen).
static inline bool ksr_plan(const uint8_t* msgs, const uint64_t* off, size_t n_groups, size_t C, KsrPlan& p, std::vector<uint32_t>& start,
                            std::vector<uint32_t>& len) {
  p.order.resize(n_groups); p.pos.resize(n_groups); p.chunk_of.resize(n_groups); p.multi.assign(n_groups, 0);
  p.rep.clear(); p.chunks.clear(); p.levels.clear(); p.items_max = 1; p.n_multi = 0;
  start.clear(); len.clear();
  // classes by byte equality, in order of first appearance
  std::unordered_map<std::string_view, uint32_t> seen;
  std::vector<uint32_t> cls(n_groups);
  for (size_t g = 0; g < n_groups; ++g) {
    const size_t l = (size_t)(off[g + 1] - off[g]);
    const std::string_view m(l ? (const char*)msgs + off[g] : "", l);
    const auto it = seen.emplace(m, (uint32_t)p.rep.size());
    if (it.second) p.rep.push_back((uint32_t)g);
    cls[g] = it.first->second;
  }
  // the stable counting sort
  const size_t n_cls = p.rep.size();
  std::vector<size_t> at(n_cls + 1, 0);
  for (size_t g = 0; g < n_groups; ++g) ++at[cls[g] + 1];
  for (size_t k = 0; k < n_cls; ++k) at[k + 1] += at[k];
  std::vector<size_t> end(at.begin() + 1, at.end());
  for (size_t g = 0; g < n_groups; ++g) { p.pos[g] = (uint32_t)at[cls[g]]; p.order[at[cls[g]]++] = (uint32_t)g; }
  // chunks, and the segments of the sums
  std::vector<SegRange> seg;
  for (size_t k = 0, a = 0; k < n_cls; a = end[k], ++k)
    for (size_t s = a; s < end[k]; s += C) {
      const size_t l = std::min(C, end[k] - s);
      for (size_t i = s; i < s + l; ++i) { p.chunk_of[p.order[i]] = (uint32_t)p.chunks.size(); p.multi[p.order[i]] = l >= 2; }
      if (l >= 2) p.n_multi += l;
      p.chunks.push_back({(uint32_t)s, (uint32_t)l, (uint32_t)k});
      seg.push_back({s, s + l});
    }
  return plan_seg_levels(seg, KSR_RUN, start, len, p.levels, &p.items_max);
}
