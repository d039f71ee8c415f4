// keyset_committee_aggregate_host.cpp -- the lane functions of csrc/keyset_committee_agg.h (selection for the checked signature
// aggregation per committee of a registered key set) compiled for the host with -DBN_CHECK (every field operation asserts the
// lazy-limb interval discipline), and the plain C++ of csrc/keyset_committee_agg_plan.h, for
// tests/test_keyset_committee_aggregate_host.py: the group search, candidate bits, ragged rows, resolved indices, the argument
// walk, the layout and the repack, the lane functions run lane by lane over ONE launch [lo, lo + m) as the kernels of
// k_keyset_committee_agg.hip index them.  TEST TOOL ONLY.
#include "../../bls-bn254_amd/csrc/keyset_committee_agg.h"
#include <cstring>
#include <string>

using namespace bn;

namespace {
KcTable g_tab;
}

extern "C" {

// the committee table the calls below work on; 0, or -1 with the text in err (256 bytes)
int hs_kca_table(const uint32_t* members, const uint64_t* com_off, size_t n_com, size_t n_keys, char* err) {
  std::string e;
  if (kc_build_table(members, com_off, n_com, n_keys, g_tab, e)) return 0;
  std::strncpy(err, e.c_str(), 255); err[255] = 0;
  return -1;
}
// coms[4 c ..] = {off, size, wbase, 0} of committee c, as the kernels read them
void hs_kca_coms(uint32_t* coms) {
  for (size_t c = 0; c < g_tab.com.size(); ++c) { coms[4 * c] = g_tab.com[c].off; coms[4 * c + 1] = g_tab.com[c].size; coms[4 * c + 2] = g_tab.com[c].wbase; coms[4 * c + 3] = 0; }
}

// kca_group for the entries lo .. lo + m
void hs_kca_groups(const uint32_t* goff, uint32_t ng, uint32_t lo, uint32_t m, uint32_t* out) {
  for (uint32_t i = 0; i < m; ++i) out[i] = kca_group(goff, ng, lo + i);
}

// k_kca_scan: cand[i] for the lanes of the launch (one byte each; the kernel packs them by ballot) and ident[i] = the point the
// lane stores is the identity (z == 0)
void hs_kca_scan(const uint32_t* cvalid, const uint32_t* com, const uint32_t* goff, uint32_t ng, const uint32_t* pos, const uint8_t* sigs, const uint8_t* mask,
                 uint32_t lo, uint32_t m, uint8_t* cand, uint8_t* ident) {
  for (uint32_t i = 0; i < m; ++i) {
    const size_t s = (size_t)lo + i;
    const KcCom& k = g_tab.com[com[kca_group(goff, ng, (uint32_t)s)]];
    const KaScan r = kca_scan(cvalid + k.wbase, pos, sigs, mask, s);
    cand[i] = r.cand ? 1 : 0;
    ident[i] = fp_is_zero(r.p.z) ? 1 : 0;
  }
}

// k_kca_rows: lanes lo .. lo + m of the wpre[ng] word lanes into rows (untouched bytes keep what the caller put there)
void hs_kca_rows(const uint32_t* pos, const uint8_t* cand, const uint32_t* goff, const uint64_t* wpre, const uint64_t* roff, const uint32_t* com, uint32_t ng,
                 uint64_t lo, uint32_t m, uint8_t* rows) {
  for (uint32_t i = 0; i < m; ++i) {
    const uint64_t t = lo + i;
    const uint32_t g = kca_word_group(wpre, ng, t), w = (uint32_t)(t - wpre[g]);
    ka_row_store(rows + roff[g], ks_row_bytes(g_tab.com[com[g]].size), w, ka_row_word(pos, cand, goff[g], goff[g + 1], w));
  }
}

// k_kca_resolve: entries lo .. lo + m
void hs_kca_resolve(const uint32_t* members, const uint32_t* com, const uint32_t* goff, uint32_t ng, const uint32_t* pos, uint32_t lo, uint32_t m, uint32_t* idx) {
  for (uint32_t i = 0; i < m; ++i) {
    const size_t s = (size_t)lo + i;
    idx[s] = kca_resolve(members + g_tab.com[com[kca_group(goff, ng, (uint32_t)s)]].off, pos, s);
  }
}

// kca_walk: the code; where[0] = group, where[1] = entry
int hs_kca_walk(const uint32_t* com, const uint32_t* pos, const uint64_t* sig_off, const uint64_t* sel_off, size_t n_groups, uint64_t max_entries, uint64_t* where) {
  const KcaWalk r = kca_walk(g_tab, com, pos, sig_off, sel_off, n_groups, max_entries);
  where[0] = r.group; where[1] = r.entry;
  return (int)r.code;
}

// kca_layout: wpre / roff hold n_groups + 1 entries each
void hs_kca_layout(const uint32_t* com, const uint64_t* sel_off, size_t n_groups, uint64_t* wpre, uint64_t* roff) {
  std::vector<uint64_t> a, b;
  kca_layout(g_tab, com, sel_off, n_groups, a, b);
  std::memcpy(wpre, a.data(), 8 * a.size()); std::memcpy(roff, b.data(), 8 * b.size());
}

// kca_repack: returns the sub-call's entry count; pos_out / src_out hold room for every entry of the call, com_out for n_fail,
// off_out / sel_off_out for n_fail + 1
size_t hs_kca_repack(const uint64_t* fail, size_t n_fail, const uint32_t* com, const uint32_t* pos, const uint64_t* sig_off, const uint64_t* sel_off,
                     const uint8_t* rows, uint32_t* com_out, uint32_t* pos_out, uint64_t* src_out, uint64_t* off_out, uint64_t* sel_off_out) {
  KcaRepack r;
  kca_repack(std::vector<size_t>(fail, fail + n_fail), com, pos, sig_off, sel_off, rows, r);
  if (!r.pos.empty()) {
    std::memcpy(pos_out, r.pos.data(), 4 * r.pos.size());
    std::memcpy(src_out, r.src.data(), 8 * r.src.size());
  }
  if (!r.com.empty()) std::memcpy(com_out, r.com.data(), 4 * r.com.size());
  std::memcpy(off_out, r.off.data(), 8 * r.off.size());
  std::memcpy(sel_off_out, r.sel_off.data(), 8 * r.sel_off.size());
  return r.pos.size();
}

}  // extern "C"
