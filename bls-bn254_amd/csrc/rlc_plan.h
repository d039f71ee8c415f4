// rlc_plan.h -- what the host decides WITHOUT the device in the batch verification by random linear combination (host_rlc.hip,
// DESIGN.md 5): whether a batch's keys repeat, the chunk size, the bounds a chunk count read back from the device must lie in,
// and the back-off of the key round.  Plain C++ over the standard library only (no HIP, no context), so that
// tests/hostsim/rlc_plan_host.cpp compiles it for the CPU against a Python model.
#pragma once
#include <cstddef>
#include <cstdint>

#include "launch_forms.h"    // LaunchForms: the lanes of a round and the limits of the quad and wave forms

static const size_t RLC_DEFAULT_GROUP = 16;    // tuples per chunk unless blsbn254_set_rlc_group / BLSBN254_RLC_GROUP says otherwise
static const size_t RLC_MAX_GROUP = 4096;      // the largest chunk either of them takes
static const unsigned RLC_MAX_STREAK = 4;      // the back-off doubles up to 2^4 = 16 skipped calls

// The chunked path is taken when the keys repeat: u distinct keys among n tuples, every key owning two tuples on average, and
// no more keys than the prepared-key tables address.  (aggregate_rlc_plan.h agr_keys_repeat is this rule with the signatures'
// pair as one key more.)
static inline bool rlc_keys_repeat(size_t n, size_t u, size_t max_keys) { return u * 2 <= n && u <= max_keys; }

// The chunks of `items` items in runs of u keys cut into pieces of at most G: at most items / G full ones and one short one per key
static inline size_t rlc_chunk_bound(size_t items, size_t G, size_t u) { return items / G + u; }

// Chunk size.  A caller's explicit setting is taken as it is.  Otherwise, from `group`:
//   1. the chunk round runs one wave per SIMD, i.e. lanes_per_round virtual tuples at a time, and a launch that is a few chunks
//      over a multiple of that pays a whole extra round: if the bound n / G + u needs more than one round, take the first g in
//      G + 1 .. 2 G whose bound needs a round less;
//   2. up to tri_max virtual tuples a round runs three lanes per tuple (k_tri.hip: less than half the latency of the
//      lane-per-tuple kernels): if those kernels are enabled (both quad halves, and tri_max above the wave-per-tuple limit) and
//      the bound of the G chosen so far is above tri_max, take the first g in G + 1 .. 2 G whose bound is not (262144 tuples
//      over 1024 keys: G = 18 -> at most 15587 chunks instead of 17408).
// The numbers are LaunchForms' (launch_forms.h): R = lanes_per_round, tri = both quad halves on, the two limits.  Written over the
// numbers so that the host program drives exactly this body; host_rlc.hip calls the overload below with the context's forms.
static inline size_t rlc_chunk_size(size_t n, size_t u, size_t group, bool group_auto, size_t R, bool tri, size_t tri_max, size_t wide_max) {
  size_t G = group;
  if (!group_auto) return G;
  const size_t r0 = (rlc_chunk_bound(n, G, u) + R - 1) / R;
  for (size_t g = G + 1; r0 > 1 && g <= 2 * G; ++g)
    if ((rlc_chunk_bound(n, g, u) + R - 1) / R < r0) { G = g; break; }
  if (tri && tri_max > wide_max && rlc_chunk_bound(n, G, u) > tri_max)
    for (size_t g = G + 1; g <= 2 * G; ++g)
      if (rlc_chunk_bound(n, g, u) <= tri_max) { G = g; break; }
  return G;
}
static inline size_t rlc_chunk_size(size_t n, size_t u, size_t group, bool group_auto, const LaunchForms& F) {
  return rlc_chunk_size(n, u, group, group_auto, F.lanes_per_round, F.tri_miller && F.tri_fe, F.tri_max, F.wide_max);
}

// What comes back from the device is checked before anything is sized by it.  The chunks of n tuples: at least one, and no more
// than tuples
static inline bool rlc_chunks_in_range(size_t m, size_t n) { return m != 0 && m <= n; }
// ... the chunks of a level of key_sums over `items` items of u keys, m_max = rlc_chunk_bound(items of level 0, G, u): every
// key has one (an empty key too), never more than the level's items or than what was reserved
static inline bool rlc_level_in_range(size_t m, size_t u, size_t m_max, size_t items) { return m >= u && m <= m_max && m <= items; }
// ... the chunks of the keys that failed the key round, of m chunks: the round failed, so at least one
static inline bool rlc_list_in_range(size_t mc, size_t m) { return mc != 0 && mc <= m; }
// ... the tuples sent to the exact round, of n
static inline bool rlc_fallback_in_range(size_t m2, size_t n) { return m2 <= n; }

// The back-off of the key round.  Batches that keep failing it (a stream with invalid signatures spread over all keys) would pay
// for it every time: after a failure the next 2 (then 4, 8, 16) calls skip it; a pass resets the back-off.  A context whose key
// round is switched off (enabled == false) neither takes it nor counts the call as skipped.
struct RlcBackoff {
  unsigned skip = 0, streak = 0;      // calls still to skip; consecutive failures, capped at RLC_MAX_STREAK
  bool take(bool enabled) {           // once per call: take the key round this call?
    if (!enabled) return false;
    if (skip) { --skip; return false; }
    return true;
  }
  void passed() { streak = 0; }
  void failed() { if (streak < RLC_MAX_STREAK) ++streak; skip = 1u << streak; }
  void reset() { skip = streak = 0; }
};
