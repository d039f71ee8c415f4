// keyset_merge_plan.h -- the host side of the checked merge of partial aggregates over a registered key set that needs neither
// HIP nor the context (host_keyset_merge.hip; the lane functions are in keyset_merge.h): the walk over a call's offsets, limits
// and rows, and the repack of the groups that go to the per-contribution fallback.  Plain C++ over the standard library only,
// as keyset_agg_plan.h, so that tests/hostsim/keyset_merge_host.cpp compiles it for the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

// The walk over the call's offsets and rows: KM_OK, or the first thing that is wrong and where.  rows is indexed by the offsets
// themselves (which need not start at 0), row s being the ceil(n_keys / 8) bytes at rows + s * row_bytes; max_con bounds
// con_off[n_groups] - con_off[0], max_row_bytes the bytes of those rows together.  KM_ROW_PAD: a row sets a bit at an index
// >= n_keys, which can only be in its last byte.
enum KmWalkCode { KM_OK = 0, KM_OFF_DECREASE, KM_TOO_MANY, KM_ROWS_TOO_LARGE, KM_ROW_PAD };
struct KmWalk { KmWalkCode code; size_t group; uint64_t con; };
static inline KmWalk km_walk(const uint8_t* rows, const uint64_t* con_off, size_t n_groups, size_t n_keys, uint64_t max_con, uint64_t max_row_bytes) {
  for (size_t g = 0; g < n_groups; ++g)
    if (con_off[g + 1] < con_off[g]) return {KM_OFF_DECREASE, g, con_off[g]};
  const uint64_t N = con_off[n_groups] - con_off[0], rb = (n_keys + 7) / 8;
  if (N > max_con) return {KM_TOO_MANY, 0, 0};
  if (N * rb > max_row_bytes) return {KM_ROWS_TOO_LARGE, 0, 0};
  if (n_keys & 7) {
    const uint8_t pad = (uint8_t)(0xffu << (n_keys & 7));
    for (size_t g = 0; g < n_groups; ++g)
      for (uint64_t s = con_off[g]; s < con_off[g + 1]; ++s)
        if (rows[s * rb + rb - 1] & pad) return {KM_ROW_PAD, g, s};
  }
  return {KM_OK, 0, 0};
}
// The sub-call of the groups in `fail` (ascending group numbers of the call): of each group the CANDIDATE contributions only,
// in the order given.  cand: the candidate bitmap over the call's contributions (bit s - con_off[0], LSB-first).  pos: the call
// position (an index into the caller's rows / sigs) each one came from; off: the sub-call's offsets, from 0; rows / sigs: their
// rows and signatures, contiguous.  sig_bytes: the size of one signature as the caller holds it (64, or 32 in wire format).
struct KmRepack { std::vector<uint64_t> pos, off; std::vector<uint8_t> rows, sigs; };
static inline void km_repack(const std::vector<size_t>& fail, const uint8_t* rows, const uint8_t* sigs, const uint64_t* con_off, const uint8_t* cand,
                             size_t row_bytes, KmRepack& out, size_t sig_bytes = 64) {
  out.pos.clear(); out.off.assign(1, 0);
  for (size_t g : fail) {
    for (uint64_t s = con_off[g]; s < con_off[g + 1]; ++s) {
      const uint64_t b = s - con_off[0];
      if ((cand[b >> 3] >> (b & 7)) & 1) out.pos.push_back(s);
    }
    out.off.push_back(out.pos.size());
  }
  const size_t n = out.pos.size();
  out.rows.resize(n * row_bytes); out.sigs.resize(sig_bytes * n);
  for (size_t i = 0; i < n; ++i) {
    std::memcpy(out.rows.data() + i * row_bytes, rows + out.pos[i] * row_bytes, row_bytes);
    std::memcpy(out.sigs.data() + sig_bytes * i, sigs + sig_bytes * out.pos[i], sig_bytes);
  }
}
