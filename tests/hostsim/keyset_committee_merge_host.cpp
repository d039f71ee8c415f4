// keyset_committee_merge_host.cpp -- the lane functions of csrc/keyset_committee_merge.h (selection for the checked merge of
// partial aggregates per committee of a registered key set, over the lane functions of csrc/keyset_merge.h) compiled for the
// host with -DBN_CHECK, and the plain C++ of csrc/keyset_committee_merge_plan.h, for tests/test_keyset_committee_merge_host.py.
// A wave of k_kcm_select is run as 64 lane states in LOCKSTEP: every lane's share of the votes is computed before any lane acts
// on them, and this harness, standing in for __any, ORs the shares.  TEST TOOL ONLY.
#include "../../bls-bn254_amd/csrc/keyset_committee_merge.h"
#include <cstring>
#include <string>

using namespace bn;

namespace {
KcTable g_tab;
}

extern "C" {

// the committee table the calls below work on; 0, or -1 with the text in err (256 bytes)
int hs_kcm_table(const uint32_t* members, const uint64_t* com_off, size_t n_com, size_t n_keys, char* err) {
  std::string e;
  if (kc_build_table(members, com_off, n_com, n_keys, g_tab, e)) return 0;
  std::strncpy(err, e.c_str(), 255); err[255] = 0;
  return -1;
}
// wbase[c] = the base of committee c's words, where its validity words lie in cvalid
void hs_kcm_wbase(uint32_t* wbase) {
  for (size_t c = 0; c < g_tab.com.size(); ++c) wbase[c] = g_tab.com[c].wbase;
}

// k_kcm_select over the groups g_lo .. g_lo + m of the call, a wave each, as the kernel indexes them: flags (a byte per
// contribution of those groups) and the groups' merged rows (untouched bytes keep what the caller put there)
void hs_kcm_select(const uint8_t* rows, const uint8_t* sig_ok, const uint8_t* mask, const uint32_t* goff, const uint32_t* com, const uint32_t* cvalid,
                   const uint64_t* rbase, const uint64_t* roff, uint32_t g_lo, uint32_t m, uint8_t* flags, uint8_t* urows) {
  for (uint32_t g = g_lo; g < g_lo + m; ++g) {
    const KcCom& k = g_tab.com[com[g]];
    const KcmGroup v = kcm_group(k.size, k.wbase, cvalid, goff, rbase, roff, g, rows, urows);
    uint32_t ureg[KM_WAVE];
    for (uint32_t l = 0; l < KM_WAVE; ++l) km_begin(v.urow, v.rb, v.W, l, ureg[l]);
    for (uint32_t s = v.a; s < v.b; ++s) {
      const uint8_t* row = kcm_row(v, s);
      KmVote any{false, false, false};
      for (uint32_t l = 0; l < KM_WAVE; ++l) {
        const KmVote t = km_test(row, v.rb, v.W, l, v.valid, v.urow, ureg[l]);
        any.some |= t.some; any.invalid |= t.invalid; any.overlap |= t.overlap;
      }
      const uint8_t f = km_flags(sig_ok[s] != 0, mask ? tc_bit(mask, s) : true, any);
      if (f & KM_USED)
        for (uint32_t l = 0; l < KM_WAVE; ++l) km_take(row, v.rb, v.W, l, v.urow, ureg[l]);
      flags[s] = f;
    }
    for (uint32_t l = 0; l < KM_WAVE; ++l) km_end(v.urow, v.rb, v.W, l, ureg[l]);
  }
}

// kcm_walk: the code; where[0] = group, where[1] = contribution, where[2] = the array that decreases
int hs_kcm_walk(const uint32_t* com, const uint8_t* rows, const uint64_t* row_off, const uint64_t* con_off, const uint64_t* sel_off, size_t n_groups,
                uint64_t max_con, uint64_t max_row_bytes, uint64_t* where) {
  const KcmWalk r = kcm_walk(g_tab, com, rows, row_off, con_off, sel_off, n_groups, max_con, max_row_bytes);
  where[0] = r.group; where[1] = r.con; where[2] = (uint64_t)r.which;
  return (int)r.code;
}

// kcm_layout: rbase / roff hold n_groups + 1 entries each
void hs_kcm_layout(const uint64_t* row_off, const uint64_t* sel_off, size_t n_groups, uint64_t* rbase, uint64_t* roff) {
  std::vector<uint64_t> a, b;
  kcm_layout(row_off, sel_off, n_groups, a, b);
  std::memcpy(rbase, a.data(), 8 * a.size()); std::memcpy(roff, b.data(), 8 * b.size());
}
// kcm_layout_contributions: returns the contribution count; ccom holds room for every contribution, coff for one more
size_t hs_kcm_layout_contributions(const uint32_t* com, const uint64_t* con_off, size_t n_groups, uint32_t* ccom, uint64_t* coff) {
  std::vector<uint32_t> a; std::vector<uint64_t> b;
  kcm_layout_contributions(g_tab, com, con_off, n_groups, a, b);
  if (!a.empty()) std::memcpy(ccom, a.data(), 4 * a.size());
  std::memcpy(coff, b.data(), 8 * b.size());
  return a.size();
}

// kcm_repack: returns the sub-call's contribution count; pos_out / sigs_out hold room for every contribution of the call,
// rows_out for every row byte, com_out for n_fail, off_out / row_off_out / sel_off_out for n_fail + 1
size_t hs_kcm_repack(const uint64_t* fail, size_t n_fail, const uint32_t* com, const uint8_t* rows, const uint64_t* row_off, const uint8_t* sigs,
                     const uint64_t* con_off, const uint8_t* cand, uint32_t* com_out, uint64_t* pos_out, uint64_t* off_out, uint64_t* row_off_out,
                     uint64_t* sel_off_out, uint8_t* rows_out, uint8_t* sigs_out) {
  KcmRepack r;
  kcm_repack(g_tab, std::vector<size_t>(fail, fail + n_fail), com, rows, row_off, sigs, con_off, cand, r);
  if (!r.pos.empty()) {
    std::memcpy(pos_out, r.pos.data(), 8 * r.pos.size());
    std::memcpy(rows_out, r.rows.data(), r.rows.size());
    std::memcpy(sigs_out, r.sigs.data(), r.sigs.size());
  }
  if (!r.com.empty()) std::memcpy(com_out, r.com.data(), 4 * r.com.size());
  std::memcpy(off_out, r.off.data(), 8 * r.off.size());
  std::memcpy(row_off_out, r.row_off.data(), 8 * r.row_off.size());
  std::memcpy(sel_off_out, r.sel_off.data(), 8 * r.sel_off.size());
  return r.pos.size();
}

}  // extern "C"
