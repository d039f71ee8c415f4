// keyset_agg_plan.h -- the host side of the checked signature aggregation over a registered key set that needs neither HIP nor
// the context (host_keyset_agg.hip; the lane functions are in keyset_agg.h): the walk over a call's offsets and key indices,
// and the repack of the groups that go to the per-signature fallback.  Plain C++ over the standard library only, as
// seg_plan.h, so that tests/hostsim/keyset_aggregate_host.cpp compiles it for the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

// The walk over the call's offsets and indices: KA_OK, or the first thing that is wrong and where.  idx is indexed by the
// offsets themselves (which need not start at 0); max_entries bounds sig_off[n_groups] - sig_off[0].
enum KaWalkCode { KA_OK = 0, KA_OFF_DECREASE, KA_TOO_MANY, KA_IDX_RANGE, KA_IDX_ORDER };
struct KaWalk { KaWalkCode code; size_t group; uint64_t entry; };
static inline KaWalk ka_walk(const uint32_t* idx, const uint64_t* sig_off, size_t n_groups, size_t n_keys, uint64_t max_entries) {
  for (size_t g = 0; g < n_groups; ++g)
    if (sig_off[g + 1] < sig_off[g]) return {KA_OFF_DECREASE, g, sig_off[g]};
  if (sig_off[n_groups] - sig_off[0] > max_entries) return {KA_TOO_MANY, 0, 0};
  for (size_t g = 0; g < n_groups; ++g)
    for (uint64_t s = sig_off[g]; s < sig_off[g + 1]; ++s) {
      if (idx[s] >= n_keys) return {KA_IDX_RANGE, g, s};
      if (s > sig_off[g] && idx[s] <= idx[s - 1]) return {KA_IDX_ORDER, g, s};
    }
  return {KA_OK, 0, 0};
}
// The sub-call of the groups in `fail` (ascending group numbers of the call): of each group the CANDIDATE entries only, which
// are the entries whose key's bit is set in the group's row (indices do not repeat inside a group).  idx: their key indices;
// pos: the call position (an index into the caller's idx / sigs) each one came from; off: the sub-call's offsets, from 0.
struct KaRepack { std::vector<uint32_t> idx; std::vector<uint64_t> pos, off; };
static inline void ka_repack(const std::vector<size_t>& fail, const uint32_t* idx, const uint64_t* sig_off, const uint8_t* rows, size_t row_bytes, KaRepack& out) {
  out.idx.clear(); out.pos.clear(); out.off.assign(1, 0);
  for (size_t g : fail) {
    const uint8_t* row = rows + g * row_bytes;
    for (uint64_t s = sig_off[g]; s < sig_off[g + 1]; ++s)
      if ((row[idx[s] >> 3] >> (idx[s] & 7)) & 1) { out.idx.push_back(idx[s]); out.pos.push_back(s); }
    out.off.push_back(out.idx.size());
  }
}
