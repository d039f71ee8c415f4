// keyset_weight_plan.h -- the host side of the stake weights over a registered key set that needs neither HIP nor the context
// (host_keyset_weight.hip; the lane functions are in keyset_weight.h): the check that no column of a table can overflow a sum,
// the quorum rule, the split of a call's groups over launches, and the repack of the groups that reach quorum into the sub-call
// that is summed and paired.  Plain C++ over the standard library only, as keyset_merge_plan.h, so that
// tests/hostsim/keyset_weight_host.cpp compiles it for the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

constexpr size_t KW_MAX_COLS = 8;                // BLSBN254_KS_MAX_COLS
constexpr size_t KW_WAVE_LANES = 64;             // lanes that share a group (keyset_weight.h KW_WAVE)

// weights[q * n_keys + i]: -1 when the sum of every column over ALL n_keys entries fits 64 bits, else the first column whose
// sum does not.  A table that passes cannot overflow any later sum: a row's weight is a sub-sum of a column's.
static inline int kw_overflowing_column(const uint64_t* weights, size_t n_keys, size_t n_cols) {
  for (size_t q = 0; q < n_cols; ++q) {
    uint64_t s = 0;
    for (size_t i = 0; i < n_keys; ++i)
      if (__builtin_add_overflow(s, weights[q * n_keys + i], &s)) return (int)q;
  }
  return -1;
}
// the caller's table (column-major, weights[q * n_keys + i]) as the device holds it: key-major, out[i * n_cols + q]
static inline void kw_key_major(const uint64_t* weights, size_t n_keys, size_t n_cols, std::vector<uint64_t>& out) {
  out.resize(n_keys * n_cols);
  for (size_t q = 0; q < n_cols; ++q)
    for (size_t i = 0; i < n_keys; ++i) out[i * n_cols + q] = weights[q * n_keys + i];
}
// a group reaches quorum when every column of its weights is at least the column's minimum (a minimum of 0 switches a column off)
static inline bool kw_reaches(const uint64_t* w, const uint64_t* min_weight, size_t n_cols) {
  for (size_t q = 0; q < n_cols; ++q)
    if (w[q] < min_weight[q]) return false;
  return true;
}
// the groups of a call that reach quorum, ascending: weights[g * n_cols + q]
static inline void kw_reaching(const uint64_t* weights, const uint64_t* min_weight, size_t n_groups, size_t n_cols, std::vector<size_t>& out) {
  out.clear();
  for (size_t g = 0; g < n_groups; ++g)
    if (kw_reaches(weights + g * n_cols, min_weight, n_cols)) out.push_back(g);
}
// groups of one launch of the weight kernel, a wave each: launches end on group boundaries, at most chunk / 64 groups each
static inline size_t kw_launch_groups(size_t chunk) { return chunk / KW_WAVE_LANES ? chunk / KW_WAVE_LANES : 1; }
static inline size_t kw_launches(size_t n_groups, size_t chunk) { const size_t gl = kw_launch_groups(chunk); return (n_groups + gl - 1) / gl; }
// The sub-call of the groups in `reach` (ascending group numbers of the call): their rows, signatures and messages, contiguous,
// with the message offsets from 0.  off: the call's n_groups + 1 byte offsets, which need not start at 0 (msgs is indexed by them
// as given; msgs may be null when every message is empty).
struct KwRepack { std::vector<uint8_t> rows, sigs, msgs; std::vector<uint64_t> off; };
static inline void kw_repack(const std::vector<size_t>& reach, const uint8_t* sel, size_t row_bytes, const uint8_t* msgs, const uint64_t* off,
                             const uint8_t* sigs, KwRepack& out) {
  const size_t n = reach.size();
  out.rows.resize(n * row_bytes); out.sigs.resize(64 * n); out.msgs.clear(); out.off.assign(1, 0);
  for (size_t j = 0; j < n; ++j) {
    const size_t g = reach[j];
    std::memcpy(out.rows.data() + j * row_bytes, sel + g * row_bytes, row_bytes);
    std::memcpy(out.sigs.data() + 64 * j, sigs + 64 * g, 64);
    if (off[g + 1] != off[g]) out.msgs.insert(out.msgs.end(), msgs + off[g], msgs + off[g + 1]);
    out.off.push_back(out.msgs.size());
  }
}
// bit j of the sub-call's bitmap to bit reach[j] of the call's (LSB-first); the call's bitmap is all zero before
static inline void kw_scatter_bits(const std::vector<size_t>& reach, const uint8_t* sub_bits, uint8_t* bitmap) {
  for (size_t j = 0; j < reach.size(); ++j)
    if ((sub_bits[j >> 3] >> (j & 7)) & 1) bitmap[reach[j] >> 3] |= (uint8_t)(1u << (reach[j] & 7));
}
