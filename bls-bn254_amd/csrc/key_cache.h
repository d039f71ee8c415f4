// key_cache.h -- what ONE lane does in the per-context store of prepared keys (k_keycache.hip, host_verify.hip prepare_keys), and the hash /
// comparison of the 128-byte key encodings that the batch de-duplication (k_keyprep.hip) shares with it.
// The store has room for R keys: their encodings (R x 128 B), their expanded pair tables, one validity byte each, and an
// open-addressing slot table of M >= 2 R entries (M a power of two) whose entries are store indices (KC_EMPTY: free).  Store
// indices are handed out in order of arrival: the store is filled from 0 upwards and never has holes, so `count` describes it.
// It is meant to hold C <= R keys; R is C or, if larger, the largest key capacity a call was enqueued with, so that an empty
// store takes any one batch.
// Per call, over the batch's distinct keys (the representatives of the de-duplication):
//   kc_begin    one lane: can the batch be appended (count + batch <= C)?  If not the store is emptied first -- the flag makes
//               the grid kernel behind it clear the slot table -- which costs one batch of misses, the cost without a store.
//               The rule counts the batch's keys, not its misses (those are not known yet): a key set stays resident from
//               call to call when it is at most HALF of C.
//   kc_lookup   one lane per distinct key: probe by key_hash; a slot that an EARLIER kernel filled (index < the count at the
//               begin of the call) is compared in full, 128 bytes; a slot claimed during this kernel belongs to another key of
//               the same batch -- distinct by construction -- and is skipped without reading its bytes (they may not be written
//               yet).  An empty slot ends the probe: linear probing without deletion never leaves a resident key behind one.
//               A miss takes the next index of the miss list (one atomic), which is also its store index, count + m.
//   kc_end      one lane, after the misses' tables are in place: count += misses; the running totals of hits, misses and resets
// Atomics are behind KC_LOAD / KC_CAS / KC_ADD: tests/hostsim/key_cache_host.cpp runs the same functions lane by lane on the
// host against a Python model.  They are not a CPU fallback: nothing in the product's host path calls them.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KC_HD __host__ __device__
#else
#define KC_HD
#endif

namespace bn {

constexpr uint32_t KC_EMPTY = 0xffffffffu;
// the store's device-side words: keys resident, this call's misses, this call's reset flag, this call's batch keys
enum { KC_COUNT = 0, KC_MISS = 1, KC_RESET = 2, KC_BATCH = 3, KC_STATE_WORDS = 4 };
// ... and its 64-bit running totals
enum { KC_STAT_HITS = 0, KC_STAT_MISSES = 1, KC_STAT_RESETS = 2, KC_STAT_WORDS = 3 };

#if defined(__HIP_DEVICE_COMPILE__)
#define KC_LOAD(p) __atomic_load_n((p), __ATOMIC_RELAXED)
#define KC_CAS(p, expect, val) atomicCAS((p), (expect), (val))
#define KC_ADD(p, v) atomicAdd((p), (v))
#else                                            // the host runs the lanes one after the other
KC_HD inline uint32_t kc_seq_cas(uint32_t* p, uint32_t expect, uint32_t val) { const uint32_t old = *p; if (old == expect) *p = val; return old; }
KC_HD inline uint32_t kc_seq_add(uint32_t* p, uint32_t v) { const uint32_t old = *p; *p = old + v; return old; }
#define KC_LOAD(p) (*(p))
#define KC_CAS(p, expect, val) ::bn::kc_seq_cas((p), (expect), (val))
#define KC_ADD(p, v) ::bn::kc_seq_add((p), (v))
#endif

KC_HD inline uint32_t load_u32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
KC_HD inline uint32_t key_hash(const uint8_t* pk, uint32_t seed) {
  uint32_t h = seed ^ 0x9e3779b9u;
  for (int k = 0; k < 32; ++k) { h ^= load_u32(pk + 4 * k); h *= 0x01000193u; h = (h << 13) | (h >> 19); }
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}
KC_HD inline bool key_equal(const uint8_t* a, const uint8_t* b) {
  uint32_t d = 0;
  for (int k = 0; k < 32; ++k) d |= load_u32(a + 4 * k) ^ load_u32(b + 4 * k);
  return d == 0;
}

// batch_cnt: the batch's distinct keys as counted on the device; bound: the keys the launch was sized for (<= R)
KC_HD inline void kc_begin(uint32_t* st, unsigned long long* stats, uint32_t batch_cnt, uint32_t bound, uint32_t C, uint32_t R) {
  uint32_t b = batch_cnt < bound ? batch_cnt : bound;
  if (b > R) b = R;                              // (the host never sizes a launch beyond the room: no index past it whatever it does)
  if (C > R) C = R;
  const bool reset = st[KC_COUNT] != 0 && st[KC_COUNT] + b > C;       // count + b <= C <= R, or count = 0 and b <= R
  st[KC_BATCH] = b; st[KC_MISS] = 0; st[KC_RESET] = reset ? 1u : 0u;
  if (reset) { st[KC_COUNT] = 0; ++stats[KC_STAT_RESETS]; }
}
// slot-table entry i of the grid kernel behind kc_begin
KC_HD inline void kc_clear(const uint32_t* st, uint32_t* slots, uint32_t i) { if (st[KC_RESET]) slots[i] = KC_EMPTY; }

struct KcFound { uint32_t slot, miss; };         // miss: the key's index in the miss list, KC_EMPTY on a hit
// mask = M - 1; keys: the store's encodings; base = st[KC_COUNT], which no lane changes while lookups run
KC_HD inline KcFound kc_lookup(const uint8_t* mine, uint32_t seed, uint32_t* slots, uint32_t mask, uint8_t* keys, uint32_t base, uint32_t* miss_cnt) {
  uint32_t s = key_hash(mine, seed) & mask, id = KC_EMPTY, m = KC_EMPTY;
  for (;;) {                                     // terminates: at most R of the M >= 2 R slots are ever taken
    uint32_t old = KC_LOAD(&slots[s]);
    if (old == KC_EMPTY) {
      if (id == KC_EMPTY) {                      // not resident: the key's place in the store, its bytes put there before the slot names it
        m = KC_ADD(miss_cnt, 1u); id = base + m;
        uint32_t* o = (uint32_t*)(keys + 128 * (size_t)id);
        for (int k = 0; k < 32; ++k) o[k] = load_u32(mine + 4 * k);
      }
      old = KC_CAS(&slots[s], KC_EMPTY, id);
      if (old == KC_EMPTY) return {id, m};
    }
    if (id == KC_EMPTY && old < base && key_equal(mine, keys + 128 * (size_t)old)) return {old, KC_EMPTY};
    s = (s + 1) & mask;
  }
}
KC_HD inline void kc_end(uint32_t* st, unsigned long long* stats) {
  const uint32_t m = st[KC_MISS];
  st[KC_COUNT] += m;
  stats[KC_STAT_MISSES] += m; stats[KC_STAT_HITS] += st[KC_BATCH] - m;
}

}  // namespace bn

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
// k_keycache.hip
__global__ void k_kd_cache_begin(const uint32_t* batch_cnt, uint32_t bound, uint32_t C, uint32_t R, uint32_t* st, unsigned long long* stats);
__global__ void k_kd_cache_clear(const uint32_t* st, uint32_t* slots, uint32_t m);
__global__ void k_kd_cache_lookup(const uint8_t* pks, const uint32_t* keys, uint32_t* st, uint32_t* slots, uint32_t mask, uint32_t seed, uint8_t* store_keys,
                                  uint32_t* slot_of, uint32_t* miss_rep, uint32_t* miss_slot);
__global__ void __launch_bounds__(256) k_kd_cache_scatter(const int4* dense, const uint8_t* dense_ok, const uint32_t* miss_slot, uint32_t key_words, uint32_t* st,
                                                          unsigned long long* stats, int4* table, uint8_t* valid);
__global__ void k_kd_cache_map(const uint32_t* ids, uint32_t n, const uint32_t* slot_of, uint32_t* out);
__global__ void k_kd_cache_ok(const uint32_t* slot_of, uint32_t u, const uint8_t* valid, uint8_t* ok);
#endif
