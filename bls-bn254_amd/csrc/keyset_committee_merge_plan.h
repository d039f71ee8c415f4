// keyset_committee_merge_plan.h -- the host side of the checked merge of partial aggregates PER COMMITTEE of a registered key
// set that needs neither HIP nor the context (host_keyset_committee_merge.hip; the lane functions are in
// keyset_committee_merge.h): the walk over a call's committees, offsets, limits and rows, the ragged layout of its rows, and
// the repack of the groups that go to the per-contribution fallback.  Plain C++ over the standard library only, beside
// keyset_merge_plan.h and keyset_committee_agg_plan.h, so that tests/hostsim/keyset_committee_merge_host.cpp compiles it for the
// CPU.  See DESIGN.md 6p.
//
// A group names a committee (keyset_committee_plan.h KcTable) and brings contributions; every contribution row of the group and
// the group's merged row are as wide as the committee, rb = ceil(size / 8) bytes.  The contribution rows of a group lie back to
// back from the byte offset the caller's row_off gives the group, the merged row at the byte offset the caller's sel_off gives
// it, so both are RAGGED and in general neither aligned nor a multiple of 4 bytes long.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#include "keyset_committee_plan.h"

// The walk over the call's arguments: KCM_OK, or the first thing that is wrong and where.  rows is indexed by row_off as given
// (which need not start at 0), com by the group; max_con bounds con_off[n_groups] - con_off[0], max_row_bytes the bytes of the
// contribution rows together.  Order: the offsets of every group in con_off, row_off and sel_off (`which` = 0, 1, 2 names the
// array that decreases), the contribution count, the bytes of rows, then group by group its committee, the span of its
// contribution rows, the length of its merged row and the padding bits of its rows.  KCM_ROW_PAD: a row sets a bit at a
// position >= size, which can only be in its last byte; con = the contribution, as con_off counts it.
enum KcmWalkCode { KCM_OK = 0, KCM_OFF_DECREASE, KCM_TOO_MANY, KCM_ROWS_TOO_LARGE, KCM_COM_RANGE, KCM_ROW_SPAN, KCM_SEL_LEN, KCM_ROW_PAD };
struct KcmWalk { KcmWalkCode code; size_t group; uint64_t con; int which; };
static inline KcmWalk kcm_walk(const KcTable& t, const uint32_t* com, const uint8_t* rows, const uint64_t* row_off, const uint64_t* con_off, const uint64_t* sel_off,
                               size_t n_groups, uint64_t max_con, uint64_t max_row_bytes) {
  const uint64_t* offs[3] = {con_off, row_off, sel_off};
  for (int a = 0; a < 3; ++a)
    for (size_t g = 0; g < n_groups; ++g)
      if (offs[a][g + 1] < offs[a][g]) return {KCM_OFF_DECREASE, g, con_off[g], a};
  if (con_off[n_groups] - con_off[0] > max_con) return {KCM_TOO_MANY, 0, 0, 0};
  if (row_off[n_groups] - row_off[0] > max_row_bytes) return {KCM_ROWS_TOO_LARGE, 0, 0, 0};
  for (size_t g = 0; g < n_groups; ++g) {
    if (com[g] >= t.com.size()) return {KCM_COM_RANGE, g, con_off[g], 0};
    const uint32_t size = t.com[com[g]].size;
    const uint64_t rb = kc_row_bytes(size), cnt = con_off[g + 1] - con_off[g];
    if (row_off[g + 1] - row_off[g] != cnt * rb) return {KCM_ROW_SPAN, g, con_off[g], 0};
    if (sel_off[g + 1] - sel_off[g] != rb) return {KCM_SEL_LEN, g, con_off[g], 0};
    if (size & 7) {
      const uint8_t pad = (uint8_t)(0xffu << (size & 7));
      for (uint64_t i = 0; i < cnt; ++i)
        if (rows[row_off[g] + i * rb + rb - 1] & pad) return {KCM_ROW_PAD, g, con_off[g] + i, 0};
    }
  }
  return {KCM_OK, 0, 0, 0};
}

// The ragged layout of a call that passed the walk: rbase[g] = the byte offset of the first contribution row of group g behind
// row_off[0], roff[g] = the byte offset of its merged row behind sel_off[0] (both with a closing entry: the bytes of the call).
static inline void kcm_layout(const uint64_t* row_off, const uint64_t* sel_off, size_t n_groups, std::vector<uint64_t>& rbase, std::vector<uint64_t>& roff) {
  rbase.resize(n_groups + 1); roff.resize(n_groups + 1);
  for (size_t g = 0; g <= n_groups; ++g) {
    rbase[g] = row_off[g] - row_off[0];
    roff[g] = sel_off[g] - sel_off[0];
  }
}
// The same layout per CONTRIBUTION, for the fallback's verification of every contribution on its own as a one-row group of the
// committee path: ccom[s] = the committee of the group that owns contribution s, coff[s] = the byte offset of its row behind
// row_off[0] (coff[N] = the bytes of the call).  Contributions count from the first of the call.
static inline void kcm_layout_contributions(const KcTable& t, const uint32_t* com, const uint64_t* con_off, size_t n_groups, std::vector<uint32_t>& ccom,
                                            std::vector<uint64_t>& coff) {
  ccom.clear(); coff.assign(1, 0);
  for (size_t g = 0; g < n_groups; ++g) {
    const uint64_t rb = kc_row_bytes(t.com[com[g]].size);
    for (uint64_t s = con_off[g]; s < con_off[g + 1]; ++s) { ccom.push_back(com[g]); coff.push_back(coff.back() + rb); }
  }
}

// The sub-call of the groups in `fail` (ascending group numbers of the call): of each group the CANDIDATE contributions only,
// in the order given.  cand: the candidate bitmap over the call's contributions (bit s - con_off[0], LSB-first).  pos: the call
// position (as con_off counts) each one came from; com / off / row_off / sel_off: the sub-call's committees and offsets, the
// offsets from 0; rows / sigs: the candidates' rows and signatures, contiguous.  sig_bytes: the size of one signature as the
// caller holds it (64, or 32 in wire format).
struct KcmRepack { std::vector<uint32_t> com; std::vector<uint64_t> pos, off, row_off, sel_off; std::vector<uint8_t> rows, sigs; };
static inline void kcm_repack(const KcTable& t, const std::vector<size_t>& fail, const uint32_t* com, const uint8_t* rows, const uint64_t* row_off,
                              const uint8_t* sigs, const uint64_t* con_off, const uint8_t* cand, KcmRepack& out, size_t sig_bytes = 64) {
  out.com.clear(); out.pos.clear(); out.rows.clear(); out.sigs.clear();
  out.off.assign(1, 0); out.row_off.assign(1, 0); out.sel_off.assign(1, 0);
  for (size_t g : fail) {
    const uint64_t rb = kc_row_bytes(t.com[com[g]].size);
    for (uint64_t s = con_off[g]; s < con_off[g + 1]; ++s) {
      const uint64_t b = s - con_off[0];
      if (!((cand[b >> 3] >> (b & 7)) & 1)) continue;
      const uint8_t* row = rows + row_off[g] + (s - con_off[g]) * rb;
      out.pos.push_back(s);
      out.rows.insert(out.rows.end(), row, row + rb);
      out.sigs.insert(out.sigs.end(), sigs + sig_bytes * s, sigs + sig_bytes * s + sig_bytes);
    }
    out.com.push_back(com[g]);
    out.off.push_back(out.pos.size());
    out.row_off.push_back(out.rows.size());
    out.sel_off.push_back(out.sel_off.back() + rb);
  }
}
