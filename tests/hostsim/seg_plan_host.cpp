// seg_plan_host.cpp -- the planners of the segmented reductions over ragged groups (csrc/seg_plan.h: plan_seg_levels,
// plan_launches_cut, plan_launches_whole) behind a C interface, for tests/test_seg_plan_host.py.  The header is plain C++, so
// this is the code the library runs.  A call plans into the variables below; hs_seg_read copies the plan out.  TEST TOOL ONLY.
#include "../../bls-bn254_amd/csrc/seg_plan.h"

namespace {
std::vector<uint32_t> g_start, g_len;
// items_max, m_max, the number of launches, then per launch: lo, hi, ga, gb, carry, the number of levels, {first, count} per level
std::vector<uint64_t> g_plan;

void reset() { g_start.clear(); g_len.clear(); g_plan.clear(); }
void put(const std::vector<SegLaunch>& launches, size_t items_max, size_t m_max) {
  g_plan = {items_max, m_max, launches.size()};
  for (const SegLaunch& L : launches) {
    g_plan.insert(g_plan.end(), {L.lo, L.hi, L.ga, L.gb, L.carry ? 1u : 0u, L.levels.size()});
    for (const SegLevel& P : L.levels) g_plan.insert(g_plan.end(), {P.first, P.count});
  }
}
}  // namespace

extern "C" {

// each returns the number of words of the plan, or -1 where the planner reports no convergence

// ranges: ne pairs (a, b); the plan is ONE launch {0, 0, 0, ne, 0, levels}
long hs_seg_levels(const uint64_t* ranges, size_t ne, size_t G) {
  reset();
  std::vector<SegRange> seg(ne);
  for (size_t e = 0; e < ne; ++e) seg[e] = {ranges[2 * e], ranges[2 * e + 1]};
  SegLaunch L{0, 0, 0, ne, false, {}};
  size_t items_max = 1;
  if (!plan_seg_levels(seg, G, g_start, g_len, L.levels, &items_max)) return -1;
  put({L}, items_max, 0);
  return (long)g_plan.size();
}
long hs_seg_cut(const uint64_t* rel, size_t n_groups, size_t chunk, size_t G) {
  reset();
  std::vector<SegLaunch> launches;
  size_t items_max = 0;
  if (!plan_launches_cut(std::vector<uint64_t>(rel, rel + n_groups + 1), n_groups, chunk, G, launches, g_start, g_len, &items_max)) return -1;
  put(launches, items_max, 0);
  return (long)g_plan.size();
}
long hs_seg_whole(const uint32_t* rel, size_t n_groups, size_t chunk, size_t G, size_t t_big) {
  reset();
  std::vector<SegLaunch> launches;
  size_t items_max = 0, m_max = 0;
  if (!plan_launches_whole(std::vector<uint32_t>(rel, rel + n_groups + 1), n_groups, chunk, G, t_big, launches, g_start, g_len, &m_max, &items_max)) return -1;
  put(launches, items_max, m_max);
  return (long)g_plan.size();
}
size_t hs_seg_descriptors() { return g_start.size(); }
void hs_seg_read(uint32_t* start, uint32_t* len, uint64_t* plan) {
  std::copy(g_start.begin(), g_start.end(), start);
  std::copy(g_len.begin(), g_len.end(), len);
  std::copy(g_plan.begin(), g_plan.end(), plan);
}

}  // extern "C"
