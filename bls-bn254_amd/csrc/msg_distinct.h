// msg_distinct.h -- what ONE lane does in the distinct-message rule of the aggregate verify over groups (k_msg_distinct.hip,
// host_msg_distinct.hip): group g is REPEATED when two of its pairs have the same hash point, i.e. equal affine
// (x, y) as field elements.  The rule is on the points, not on the message bytes: under the try-and-increment maps two different
// messages can share a point, and the points never leave the device.
// Per call, over the N pairs of the G groups (goff: the groups' pair offsets, G + 1 entries):
//   md_key      one lane per pair: the pair's point from a limb-major workspace -- affine (x, y) or homogeneous (x : y : z), the
//               latter normalised by one inversion -- as the canonical Montgomery limbs of x and y (MD_KEY_LIMBS words, limb-major
//               with stride N).  Equality is on VALUES: the workspaces hold lazy limbs, one value has several limb patterns,
//               and only the canonical form of fp_canon is compared.
//   md_insert   one lane per pair, behind md_key: the key (group, x, y) into an open-addressing table of M = 2^k >= 2 N slots whose
//               entries are pair indices (KC_EMPTY: free).  Probe by md_slot_hash, read before the CAS (a taken slot never changes);
//               a taken slot is compared IN FULL -- the occupant's group and its 18 limbs -- so a collision of the slot hash never
//               merges two keys.  An equal occupant: dup[g] = 1, a plain byte store (every writer stores the same value).  The
//               first pair of a key to arrive owns its slot and every later one meets it before any free slot (linear probing
//               without deletion), so dup[] does not depend on the order of arrival.  The probe ends after M slots and then marks
//               the group repeated (fail closed): unreachable with M >= 2 N, reached by the host tests' tiny tables only.
// The same point in two different groups is no repeat (the group is part of the key); a pair outside [goff[0], goff[G]) belongs
// to no group and is never inserted; an empty group has no pair and is never marked.  Key validity plays no part.
// Atomics are key_cache.h's KC_LOAD / KC_CAS: tests/hostsim/msg_distinct_host.cpp runs the same functions lane by lane on the host
// against a Python model.  They are not a CPU fallback: nothing in the product's host path calls them.
#pragma once
#include "fp29.h"
#include "key_cache.h"

namespace bn {

enum : int { MD_AFFINE = 0, MD_HOMOGENEOUS = 1 };     // the form of the points a stage reads: 18 or 27 limbs per pair
constexpr int MD_KEY_LIMBS = 2 * NL;                  // canonical x, canonical y

// slots of the table for n pairs: the smallest power of two >= 2 n (n <= 2^23: at most 2^24)
KC_HD inline uint32_t md_slots(uint32_t n) {
  uint32_t m = 2;
  while (m < 2u * n && m < (1u << 31)) m <<= 1;
  return m;
}

// A coordinate as a workspace holds it: lazy limbs, limbs 0..7 within [-L, 2 L], the top limb small, |value| < 3 p
BN_INL Fp md_load(const int32_t* ws, size_t stride) {
  Fp r;
  BN_UNROLL for (int k = 0; k < NL; ++k) r.l[k] = ws[(size_t)k * stride];
  BN_TRK(set_trk(r, -1, 2, -0.02, 0.02, 3); check_actual(r, "md_load");)
  return r;
}
// pts / key: the pair's column of the workspace (stride: pairs per limb row) and of the key array (stride n)
BN_FUNC void md_key(const int32_t* pts, size_t stride, int form, int32_t* key, size_t n) {
  BN_CTX;
  Fp x = fp_canon(md_load(pts, stride)), y = fp_canon(md_load(pts + 9 * stride, stride));
  if (form == MD_HOMOGENEOUS) {
    const Fp z = fp_canon(md_load(pts + 18 * stride, stride));
    if (fp_is_zero(z)) { x = fp_zero(); y = fp_one(); }            // the identity as the encodings write it: (0, 1)
    else { const Fp zi = fp_inv(z); x = fp_canon(fp_mul(x, zi)); y = fp_canon(fp_mul(y, zi)); }
  }
  for (int k = 0; k < NL; ++k) { key[(size_t)k * n] = x.l[k]; key[(size_t)(NL + k) * n] = y.l[k]; }
}

// the group of pair i, goff[0] <= i < goff[G]: the g with goff[g] <= i < goff[g + 1] (empty groups own no pair)
KC_HD inline uint32_t md_group_of(const uint32_t* goff, uint32_t G, uint32_t i) {
  uint32_t lo = 0, hi = G - 1;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (goff[mid + 1] <= i) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// Seeded per context, as key_hash is: under the digest map the caller chooses x.  -DMD_SLOT_HASH_ZERO (tests/hostsim only)
// sends every key to slot 0.
KC_HD inline uint32_t md_slot_hash(uint32_t g, const int32_t* key, size_t n, uint32_t seed) {
#ifdef MD_SLOT_HASH_ZERO
  (void)g; (void)key; (void)n; (void)seed;
  return 0;
#else
  uint32_t h = seed ^ 0x9e3779b9u;
  h ^= g; h *= 0x01000193u; h = (h << 13) | (h >> 19);
  for (int k = 0; k < MD_KEY_LIMBS; ++k) { h ^= (uint32_t)key[(size_t)k * n]; h *= 0x01000193u; h = (h << 13) | (h >> 19); }
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
#endif
}
KC_HD inline bool md_key_equal(const int32_t* a, const int32_t* b, size_t n) {
  uint32_t d = 0;
  for (int k = 0; k < MD_KEY_LIMBS; ++k) d |= (uint32_t)(a[(size_t)k * n] ^ b[(size_t)k * n]);
  return d == 0;
}
// key: the array md_key filled (stride n); mask = M - 1; slots: M entries, all KC_EMPTY before the first lane; dup: G bytes, all 0
KC_HD inline void md_insert(uint32_t i, uint32_t n, const uint32_t* goff, uint32_t G, const int32_t* key, uint32_t* slots, uint32_t mask, uint32_t seed,
                            uint8_t* dup) {
  if (G == 0 || i >= n || i < goff[0] || i >= goff[G]) return;       // in front of the first group or behind the last: no group
  const uint32_t g = md_group_of(goff, G, i), g_lo = goff[g], g_hi = goff[g + 1];
  uint32_t s = md_slot_hash(g, key + i, n, seed) & mask;
  for (uint32_t step = 0; step <= mask; ++step) {
    uint32_t old = KC_LOAD(&slots[s]);
    if (old == KC_EMPTY) old = KC_CAS(&slots[s], KC_EMPTY, i);
    if (old == KC_EMPTY) return;                                     // the first pair of its key
    if (old >= n) break;                                             // (never: the lanes write indices below n into a cleared table)
    if (old >= g_lo && old < g_hi && md_key_equal(key + i, key + old, n)) { dup[g] = 1; return; }
    s = (s + 1) & mask;
  }
  dup[g] = 1;                                                        // no free slot in M probes: fail closed
}

}  // namespace bn

#if defined(__HIPCC__)
// k_msg_distinct.hip
__global__ void __launch_bounds__(256) k_md_keys(const int32_t* pts, size_t stride, uint32_t n, int form, int32_t* key);
__global__ void __launch_bounds__(256) k_md_insert(uint32_t n, const uint32_t* goff, uint32_t G, const int32_t* key, uint32_t* slots, uint32_t mask, uint32_t seed,
                                                   uint8_t* dup);
#endif
