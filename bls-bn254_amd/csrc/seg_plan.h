// seg_plan.h -- host-side planning of the segmented reductions over ragged groups (k_fp12_seg_prod, k_g1_seg_sum, k_g2_seg_sum):
// which items a launch takes, and the (start, len) run descriptors of every level of its reduction.  Plain C++ over the standard
// library only (no HIP, no context), so that tests/hostsim/seg_plan_host.cpp compiles it for the CPU; see DESIGN.md 4b.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

struct SegLevel { size_t first, count; };   // one level of a segmented reduction: its descriptors are [first, first + count)
// One launch: items [lo, hi) of the call, groups [ga, gb) with their levels.  carry: group ga began in an earlier launch, the last
// level folds into its running value (the cut planner only; the whole-group planner never carries).
struct SegLaunch { size_t lo, hi, ga, gb; bool carry; std::vector<SegLevel> levels; };
typedef std::pair<uint64_t, uint64_t> SegRange;   // items [first, second) of one segment

// Levels of one launch.  Level 0 cuts every segment's item range seg[e] into runs of at most G items, one (start, len) descriptor
// per run (an empty segment: ONE empty run, which the kernels turn into the identity with flag 0); the runs, in order, are the next
// level's items -- contiguous by construction -- and so on until there is one run per segment.  Descriptors are appended to
// start / len, one {first descriptor, count} per level to `levels`; *items_max is raised to the largest level that is written
// to the ping-pong buffers (every level but the last, which has its own destination).  false: no convergence (cannot happen
// for G >= 2).
static inline bool plan_seg_levels(const std::vector<SegRange>& seg, size_t G, std::vector<uint32_t>& start, std::vector<uint32_t>& len,
                                   std::vector<SegLevel>& levels, size_t* items_max) {
  const size_t ne = seg.size();
  std::vector<uint64_t> cur(ne + 1), nxt(ne + 1);
  for (int level = 0; ; ++level) {
    if (level > 40) return false;
    const size_t first = start.size();
    for (size_t e = 0; e < ne; ++e) {
      const uint64_t a = level ? cur[e] : seg[e].first, b = level ? cur[e + 1] : seg[e].second;
      nxt[e] = start.size() - first;
      if (a == b) { start.push_back((uint32_t)a); len.push_back(0); }
      for (uint64_t s = a; s < b; s += G) { start.push_back((uint32_t)s); len.push_back((uint32_t)std::min<uint64_t>(b - s, G)); }
    }
    const size_t m = start.size() - first;
    nxt[ne] = m;
    levels.push_back({first, m});
    if (m == ne) return true;
    *items_max = std::max(*items_max, m);
    cur.swap(nxt);
  }
}

// Launches that may cut a group, for groups rel[0 .. n_groups] (offsets rebased to 0): at most `chunk` items each, ending at the
// last group boundary inside the window where there is one, else inside the group, which is then carried into the next launch.
// Trailing empty groups go to the last launch; no items at all: one launch of every group.
static inline bool plan_launches_cut(const std::vector<uint64_t>& rel, size_t n_groups, size_t chunk, size_t G, std::vector<SegLaunch>& out,
                                     std::vector<uint32_t>& start, std::vector<uint32_t>& len, size_t* items_max) {
  const size_t N = (size_t)rel[n_groups];
  size_t lo = 0, g = 0;
  *items_max = 1;
  do {
    SegLaunch L;
    const size_t lim = std::min(N, lo + chunk);
    // the last group boundary in (lo, lim], else lim (inside a group larger than a chunk)
    const size_t k = (size_t)(std::upper_bound(rel.begin(), rel.end(), (uint64_t)lim) - rel.begin()) - 1;
    const size_t hi = rel[k] > lo ? (size_t)rel[k] : lim;
    // groups [g, gb): the unfinished ones that begin before hi; the last launch takes every remaining (empty) one
    const size_t gb = hi == N ? n_groups : (size_t)(std::lower_bound(rel.begin(), rel.end(), (uint64_t)hi) - rel.begin());
    L.lo = lo; L.hi = hi; L.ga = g; L.gb = gb; L.carry = rel[g] < lo;
    std::vector<SegRange> seg(gb - g);
    for (size_t e = 0; e < gb - g; ++e)                  // launch-local, clamped to the launch
      seg[e] = {std::min<uint64_t>(std::max<uint64_t>(rel[g + e], lo), hi) - lo, std::min<uint64_t>(std::max<uint64_t>(rel[g + e + 1], lo), hi) - lo};
    if (!plan_seg_levels(seg, G, start, len, L.levels, items_max)) return false;
    out.push_back(std::move(L));
    g = (gb > g && rel[gb] > hi) ? gb - 1 : gb;          // a group cut at hi continues in the next launch
    lo = hi;
  } while (lo < N);
  return true;
}

// Launches of whole groups, for groups rel[0 .. n_groups] (offsets rebased to 0): a group of at most t_big items lies in exactly
// one launch (which holds at most `chunk` items unless its first group alone has more).  A larger group is the caller's to reduce:
// it may be cut anywhere and is ONE empty run (the identity) in every launch it touches.  m_max: the largest launch.
static inline bool plan_launches_whole(const std::vector<uint32_t>& rel, size_t n_groups, size_t chunk, size_t G, size_t t_big, std::vector<SegLaunch>& out,
                                       std::vector<uint32_t>& start, std::vector<uint32_t>& len, size_t* m_max, size_t* items_max) {
  const auto big = [&](size_t g) { return (size_t)(rel[g + 1] - rel[g]) > t_big; };
  const size_t N = rel[n_groups];
  size_t lo = 0, g = 0;
  *m_max = 0; *items_max = 1;
  while (g < n_groups) {
    SegLaunch L;
    const size_t lim = std::min(N, lo + chunk);
    size_t hi = lo, gb = g;
    bool cut = false;                                    // the launch ends inside the (large) group gb
    while (gb < n_groups) {
      const size_t b = rel[gb + 1];
      if (b <= lim || (hi == lo && !big(gb))) { hi = b; ++gb; if (b > lim) break; continue; }   // a whole group; the first one whatever its size
      if (big(gb) && lim > hi) { hi = lim; cut = true; }
      break;
    }
    L.lo = lo; L.hi = hi; L.ga = g; L.gb = gb + (cut ? 1 : 0); L.carry = false;
    std::vector<SegRange> seg(L.gb - L.ga);
    for (size_t e = 0; e < seg.size(); ++e) seg[e] = big(L.ga + e) ? SegRange{0, 0} : SegRange{rel[L.ga + e] - lo, rel[L.ga + e + 1] - lo};
    if (!plan_seg_levels(seg, G, start, len, L.levels, items_max)) return false;
    *m_max = std::max(*m_max, hi - lo);
    out.push_back(std::move(L));
    g = gb; lo = hi;
  }
  return true;
}
