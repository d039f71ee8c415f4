// keyset_merge_host.cpp -- the lane functions of csrc/keyset_merge.h (selection for the checked merge of partial aggregates over
// a registered key set) compiled for the host with -DBN_CHECK (every field operation asserts the lazy-limb interval discipline),
// and the plain C++ of csrc/keyset_merge_plan.h, for tests/test_keyset_merge_host.py.  A wave of k_km_select is run as 64 lane
// states in LOCKSTEP: every lane's share of the votes is computed before any lane acts on them, and this harness, standing in
// for __any, ORs the shares.  TEST TOOL ONLY.
#include "../../bls-bn254_amd/csrc/keyset_merge.h"
#include <cstring>

using namespace bn;

extern "C" {

// k_km_sig: ok[i] for the contributions lo .. lo + m and ident[i] = the point the lane stores is the identity (z == 0)
void hs_km_sig(const uint8_t* sigs, uint32_t lo, uint32_t m, uint8_t* ok, uint8_t* ident) {
  for (uint32_t i = 0; i < m; ++i) {
    const KmSig r = km_sig(sigs, (size_t)lo + i);
    ok[i] = r.ok ? 1 : 0;
    ident[i] = fp_is_zero(r.p.z) ? 1 : 0;
  }
}

// k_km_select over the groups g_lo .. g_lo + m of the call, a wave each, as the kernel indexes them: flags (a byte per
// contribution of those groups) and the groups' merged rows (untouched bytes keep what the caller put there)
void hs_km_select(const uint8_t* rows, const uint8_t* sig_ok, const uint8_t* mask, const uint32_t* goff, const uint32_t* valid, uint32_t n_keys, uint32_t g_lo,
                  uint32_t m, uint8_t* flags, uint8_t* urows) {
  const uint32_t W = ks_words(n_keys), rb = ks_row_bytes(n_keys);
  for (uint32_t g = g_lo; g < g_lo + m; ++g) {
    uint8_t* urow = urows + (size_t)g * rb;
    uint32_t ureg[KM_WAVE];
    for (uint32_t l = 0; l < KM_WAVE; ++l) km_begin(urow, rb, W, l, ureg[l]);
    for (uint32_t s = goff[g]; s < goff[g + 1]; ++s) {
      const uint8_t* row = rows + (size_t)s * rb;
      KmVote any{false, false, false};
      for (uint32_t l = 0; l < KM_WAVE; ++l) {
        const KmVote v = km_test(row, rb, W, l, valid, urow, ureg[l]);
        any.some |= v.some; any.invalid |= v.invalid; any.overlap |= v.overlap;
      }
      const uint8_t f = km_flags(sig_ok[s] != 0, mask ? tc_bit(mask, s) : true, any);
      if (f & KM_USED)
        for (uint32_t l = 0; l < KM_WAVE; ++l) km_take(row, rb, W, l, urow, ureg[l]);
      flags[s] = f;
    }
    for (uint32_t l = 0; l < KM_WAVE; ++l) km_end(urow, rb, W, l, ureg[l]);
  }
}

// k_km_points: ident[i] = the lane overwrites its point with the identity; the point it writes is checked to be one
void hs_km_points(const uint8_t* flags, uint32_t lo, uint32_t m, uint8_t* ident) {
  for (uint32_t i = 0; i < m; ++i) {
    ident[i] = 0;
    if (flags[lo + i] & KM_USED) continue;
    int32_t ws[3 * NL];
    for (int j = 0; j < 3 * NL; ++j) ws[j] = 0x5a5a;
    km_drop_point(ws, 1);
    ident[i] = fp_is_zero(load_fp(ws + 2 * NL, 1)) ? 1 : 2;
  }
}

// km_walk: the code; where[0] = group, where[1] = contribution
int hs_km_walk(const uint8_t* rows, const uint64_t* con_off, size_t n_groups, size_t n_keys, uint64_t max_con, uint64_t max_row_bytes, uint64_t* where) {
  const KmWalk r = km_walk(rows, con_off, n_groups, n_keys, max_con, max_row_bytes);
  where[0] = r.group; where[1] = r.con;
  return (int)r.code;
}

// km_repack: returns the sub-call's contribution count; pos_out / rows_out / sigs_out hold room for every contribution of the
// call, off_out for n_fail + 1
size_t hs_km_repack(const uint64_t* fail, size_t n_fail, const uint8_t* rows, const uint8_t* sigs, const uint64_t* con_off, const uint8_t* cand, size_t row_bytes,
                    uint64_t* pos_out, uint64_t* off_out, uint8_t* rows_out, uint8_t* sigs_out) {
  KmRepack r;
  km_repack(std::vector<size_t>(fail, fail + n_fail), rows, sigs, con_off, cand, row_bytes, r);
  if (!r.pos.empty()) {
    std::memcpy(pos_out, r.pos.data(), 8 * r.pos.size());
    std::memcpy(rows_out, r.rows.data(), r.rows.size());
    std::memcpy(sigs_out, r.sigs.data(), r.sigs.size());
  }
  std::memcpy(off_out, r.off.data(), 8 * r.off.size());
  return r.pos.size();
}

}  // extern "C"
