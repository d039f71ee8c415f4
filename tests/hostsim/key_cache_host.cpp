// key_cache_host.cpp -- the lane functions of csrc/key_cache.h (the store of prepared keys: begin / clear / lookup / end) run on
// the host, lane by lane in the order k_keycache.hip indexes them, over a scripted sequence of batches, for
// tests/test_key_cache_host.py, which compares every step with a Python dict model.  A stand-alone program, so that it can also be
// built with -fsanitize=address,undefined and run as it is: every buffer has exactly the size the kernels are given.  TEST TOOL ONLY.
//   usage: key_cache_host SCRIPT
//   SCRIPT: "C M seed" on the first line (capacity, slot-table entries -- a power of two >= 2 C --, hash seed), then per batch a line
//   "B k" followed by k lines of 256 hex digits (the batch's distinct keys, in the order of their batch key ids).
//   Output per batch: "batch reset count hits misses resets", "slot_of ...", "miss rep:slot ...", "table ..." (M entries, -1 = free),
//   "key <slot> <hex>" for every resident key.
#include "../../bls-bn254_amd/csrc/key_cache.h"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

using namespace bn;

static int hexval(char ch) { return ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1; }

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: key_cache_host SCRIPT\n"); return 2; }
  std::ifstream in(argv[1]);
  uint32_t C = 0, M = 0, seed = 0;
  if (!(in >> C >> M >> seed) || C == 0 || M < 2 * C || (M & (M - 1))) { std::fprintf(stderr, "bad header\n"); return 2; }
  std::vector<uint8_t> store_keys(128 * (size_t)C);
  std::vector<uint32_t> slots(M, KC_EMPTY), st(KC_STATE_WORDS, 0);
  std::vector<unsigned long long> stats(KC_STAT_WORDS, 0);
  std::string tag;
  while (in >> tag) {
    uint32_t k = 0;
    if (tag != "B" || !(in >> k)) { std::fprintf(stderr, "bad batch line\n"); return 2; }
    std::vector<uint8_t> pks(128 * (size_t)k);
    for (uint32_t j = 0; j < k; ++j) {
      std::string hex;
      if (!(in >> hex) || hex.size() != 256) { std::fprintf(stderr, "bad key\n"); return 2; }
      for (int b = 0; b < 128; ++b) {
        const int hi = hexval(hex[2 * b]), lo = hexval(hex[2 * b + 1]);
        if (hi < 0 || lo < 0) { std::fprintf(stderr, "bad key\n"); return 2; }
        pks[128 * (size_t)j + b] = (uint8_t)(16 * hi + lo);
      }
    }
    // the de-duplication's outputs for a batch of k distinct keys: key j's representative tuple is tuple j
    std::vector<uint32_t> keys(k), slot_of(k, KC_EMPTY), miss_rep(k, KC_EMPTY), miss_slot(k, KC_EMPTY);
    for (uint32_t j = 0; j < k; ++j) keys[j] = j;
    const uint32_t batch_cnt = k, bound = k;
    kc_begin(st.data(), stats.data(), batch_cnt, bound, C, C);                                                   // k_kd_cache_begin
    const uint32_t reset = st[KC_RESET];
    for (uint32_t i = 0; i < M; ++i) kc_clear(st.data(), slots.data(), i);                                    // k_kd_cache_clear
    for (uint32_t j = 0; j < bound; ++j) {                                                                    // k_kd_cache_lookup
      if (j >= st[KC_BATCH]) continue;
      const uint32_t rep = keys[j];
      const KcFound f = kc_lookup(pks.data() + 128 * (size_t)rep, seed, slots.data(), M - 1, store_keys.data(), st[KC_COUNT], &st[KC_MISS]);
      slot_of[j] = f.slot;
      if (f.miss != KC_EMPTY) { miss_rep[f.miss] = rep; miss_slot[f.miss] = f.slot; }
    }
    const uint32_t misses = st[KC_MISS];
    kc_end(st.data(), stats.data());                                                                          // the last lane of k_kd_cache_scatter
    std::printf("batch %u %u %llu %llu %llu\n", reset, st[KC_COUNT], stats[KC_STAT_HITS], stats[KC_STAT_MISSES], stats[KC_STAT_RESETS]);
    std::printf("slot_of");
    for (uint32_t j = 0; j < k; ++j) std::printf(" %d", (int)slot_of[j]);
    std::printf("\nmiss");
    for (uint32_t m = 0; m < misses; ++m) std::printf(" %d:%d", (int)miss_rep[m], (int)miss_slot[m]);
    std::printf("\ntable");
    for (uint32_t i = 0; i < M; ++i) std::printf(" %d", (int)slots[i]);
    std::printf("\n");
    for (uint32_t s = 0; s < st[KC_COUNT]; ++s) {
      std::printf("key %u ", s);
      for (int b = 0; b < 128; ++b) std::printf("%02x", store_keys[128 * (size_t)s + b]);
      std::printf("\n");
    }
  }
  return 0;
}
