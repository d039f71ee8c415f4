// aggregate_rlc_plan.h -- host-side planning of the aggregate verify over ragged groups by random linear combination
// (host_aggregate_rlc.hip): the group of every pair, the number of segments of the second round, their bounds, and
// the group ranges that go to the exact pipeline.  Plain C++ over the standard library only (no HIP, no context), so that
// tests/hostsim/aggregate_rlc_host.cpp compiles it for the CPU against a Python model.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

static const size_t AGR_MAX_SEGMENTS = 4096;   // the largest S blsbn254_set_aggregate_rlc_segments takes
static const size_t AGR_SMAX = 16;             // the default rule's cap on S (chosen by scripts/bench_aggregate_rlc.py)
// Two exact sub-calls are made one when fewer than this many lanes' worth of pairs and signatures lie between them: a sub-call
// costs about 10 ms whatever its size (the lane kernel's latency), which is what the exact pipeline takes for
// about 2^16 pairs in a call that runs anyway
static const size_t AGR_MERGE_GAP = (size_t)1 << 16;

// gidx[i] = the group of pair i (pairs counted from grp_off[0]) for the G groups grp_off[0 .. G]; empty groups own no pair
static inline void agr_pair_groups(const uint64_t* grp_off, size_t G, std::vector<uint32_t>& gidx) {
  gidx.resize((size_t)(grp_off[G] - grp_off[0]));
  for (size_t g = 0; g < G; ++g)
    for (uint64_t i = grp_off[g]; i < grp_off[g + 1]; ++i) gidx[(size_t)(i - grp_off[0])] = (uint32_t)g;
}

// Round 1 is taken when the keys repeat: the rule of rlc2_chunk_dev and aggregate_verify_grouped, u distinct keys among N pairs
// and the signatures' pair as key u of the tables
static inline bool agr_keys_repeat(size_t N, size_t u, size_t max_keys) { return u * 2 <= N && u + 1 <= max_keys; }

// The segments of round 2.  setting: 0 = the default rule S = min(s_max, N / (2 u)), 1 = no second round, 2 .. AGR_MAX_SEGMENTS
// fixes S; never more segments than groups.  Returns 1 when the round is skipped (S < 2).
static inline size_t agr_segments(size_t setting, size_t s_max, size_t N, size_t u, size_t G) {
  size_t S = setting ? setting : std::min(s_max, u ? N / (2 * u) : (size_t)0);
  S = std::min(S, G);
  return S < 2 ? 1 : S;
}

// Segment s owns the consecutive groups bound[s] .. bound[s + 1]: G groups cut into S parts whose sizes differ by at most one
// (S <= G: no segment is empty); seg_of[g] = the segment of group g
static inline void agr_cut(size_t G, size_t S, std::vector<uint32_t>& bound, std::vector<uint32_t>& seg_of) {
  bound.resize(S + 1); seg_of.resize(G);
  for (size_t s = 0; s <= S; ++s) bound[s] = (uint32_t)((uint64_t)s * G / S);
  for (size_t s = 0; s < S; ++s)
    for (size_t g = bound[s]; g < bound[s + 1]; ++g) seg_of[g] = (uint32_t)s;
}

// The group ranges [first, second) of the exact sub-calls: the failed segments (pass[s] == 0), adjacent ones merged, every range
// trimmed to its first and last eligible group (empty groups in front and behind cost the exact call a lane each and decide
// nothing); a range without an eligible group is dropped; then two ranges with fewer than merge_gap pairs and signatures between
// them (grp_off: the call's group offsets) become one.  *eligible: the eligible groups inside the ranges.
static inline void agr_failed_ranges(const std::vector<uint32_t>& bound, const uint8_t* pass, const uint8_t* elig, const uint64_t* grp_off, size_t merge_gap,
                                     std::vector<std::pair<size_t, size_t>>& out, size_t* eligible) {
  const size_t S = bound.size() - 1;
  out.clear(); *eligible = 0;
  for (size_t s = 0; s < S; ) {
    if (pass[s]) { ++s; continue; }
    size_t e = s;
    while (e < S && !pass[e]) ++e;
    size_t a = bound[s], b = bound[e];
    while (a < b && !elig[a]) ++a;
    while (b > a && !elig[b - 1]) --b;
    if (a < b) {
      const size_t gap = out.empty() ? merge_gap : (size_t)(grp_off[a] - grp_off[out.back().second]) + (a - out.back().second);
      if (gap < merge_gap) out.back().second = b;
      else out.push_back({a, b});
    }
    s = e;
  }
  for (const std::pair<size_t, size_t>& r : out)
    for (size_t g = r.first; g < r.second; ++g) *eligible += elig[g] ? 1 : 0;
}
