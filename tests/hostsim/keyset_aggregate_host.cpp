// keyset_aggregate_host.cpp -- the lane functions of csrc/keyset_agg.h (selection for the checked signature aggregation over a
// registered key set) compiled for the host with -DBN_CHECK (every field operation asserts the lazy-limb interval discipline),
// and the plain C++ of csrc/keyset_agg_plan.h, for tests/test_keyset_aggregate_host.py: candidate bits, rows, the argument
// walk and the repack, the lane functions run lane by lane over ONE launch [lo, lo + m) as the kernels of k_keyset_agg.hip
// index them.  TEST TOOL ONLY.
#include "../../bls-bn254_amd/csrc/keyset_agg.h"
#include <cstring>

using namespace bn;

extern "C" {

// k_ka_scan: cand[i] for the lanes of the launch (one byte each; the kernel packs them by ballot) and ident[i] = the point the
// lane stores is the identity (z == 0)
void hs_ka_scan(const uint8_t* key_valid, const uint32_t* idx, const uint8_t* sigs, const uint8_t* mask, uint32_t lo, uint32_t m, uint8_t* cand, uint8_t* ident) {
  for (uint32_t i = 0; i < m; ++i) {
    const KaScan r = ka_scan(key_valid, idx, sigs, mask, (size_t)lo + i);
    cand[i] = r.cand ? 1 : 0;
    ident[i] = fp_is_zero(r.p.z) ? 1 : 0;
  }
}

// k_ka_rows: lanes lo .. lo + m of n_groups x W into rows (n_groups x ceil(n_keys / 8) bytes; untouched bytes keep what the
// caller put there)
void hs_ka_rows(const uint32_t* idx, const uint8_t* cand, const uint32_t* goff, uint32_t lo, uint32_t m, uint32_t n_keys, uint8_t* rows) {
  const uint32_t W = ks_words(n_keys), rb = ks_row_bytes(n_keys);
  for (uint32_t i = 0; i < m; ++i) {
    const uint32_t t = lo + i, g = t / W, w = t - g * W;
    ka_row_store(rows + (size_t)g * rb, rb, w, ka_row_word(idx, cand, goff[g], goff[g + 1], w));
  }
}

// ka_walk: the code; where[0] = group, where[1] = entry
int hs_ka_walk(const uint32_t* idx, const uint64_t* sig_off, size_t n_groups, size_t n_keys, uint64_t max_entries, uint64_t* where) {
  const KaWalk r = ka_walk(idx, sig_off, n_groups, n_keys, max_entries);
  where[0] = r.group; where[1] = r.entry;
  return (int)r.code;
}

// ka_repack: returns the sub-call's entry count; idx_out / pos_out hold room for every entry of the call, off_out for n_fail + 1
size_t hs_ka_repack(const uint64_t* fail, size_t n_fail, const uint32_t* idx, const uint64_t* sig_off, const uint8_t* rows, size_t row_bytes,
                    uint32_t* idx_out, uint64_t* pos_out, uint64_t* off_out) {
  KaRepack r;
  ka_repack(std::vector<size_t>(fail, fail + n_fail), idx, sig_off, rows, row_bytes, r);
  if (!r.idx.empty()) {
    std::memcpy(idx_out, r.idx.data(), 4 * r.idx.size());
    std::memcpy(pos_out, r.pos.data(), 8 * r.pos.size());
  }
  std::memcpy(off_out, r.off.data(), 8 * r.off.size());
  return r.idx.size();
}

}  // extern "C"
