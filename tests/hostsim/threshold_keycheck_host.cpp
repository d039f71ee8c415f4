// threshold_keycheck_host.cpp -- the lane functions of csrc/threshold_keycheck.h (dealt key shares checked against a group's
// Feldman commitments) compiled for the host with -DBN_CHECK (every field operation asserts the lazy-limb interval
// discipline), for tests/test_threshold_keycheck_host.py: the table of the generator's multiples built row by row as
// k_g2gen_table's lanes build it, the fixed-base sum, the equality, and the whole check run lane by lane as the kernels of
// k_threshold_deal.hip and k_threshold_keycheck.hip index them.  TEST TOOL ONLY.
#include "../../bls-bn254_amd/csrc/threshold_keycheck.h"
#include <vector>

using namespace bn;

extern "C" {

int hs_kc_window_bits() { return KC_WINDOW_BITS; }
int hs_kc_windows() { return KC_WINDOWS; }
size_t hs_kc_table_limbs() { return KC_TABLE_LIMBS; }

// k_g2gen_table: KC_WINDOWS lane calls into tab (KC_TABLE_LIMBS limbs, 8-byte aligned)
void hs_kc_table(int32_t* tab) {
  for (uint32_t w = 0; w < (uint32_t)KC_WINDOWS; ++w) kc_table_lane(tab, w);
}

// [k] G2gen out of the table for the 32 big-endian bytes k, as 128 wire bytes; returns the range flag (k < r)
int hs_kc_fixed_base(const int32_t* tab, const uint8_t* k_be, uint8_t* out) {
  uint32_t k[8];
  bool ok;
  kc_share_words(k_be, k, ok);
  g2_encode(out, g2_to_affine(kc_fixed_base_lane(tab, k)));
  return ok ? 1 : 0;
}

// The equality as k_td_key_check forms it: A = the table's sum for `share` (negated when neg_a), B = g2_horner_lane over the T
// commitments (wire bytes, all valid) at `id` with `nbits` bits.  Returns kc_key_check_lane's value; *z_differs = the two
// representatives have different Z; *a_inf / *b_inf = which sides are the identity.
int hs_kc_eq(const int32_t* tab, const uint8_t* share, int neg_a, const uint8_t* commitments, uint32_t T, const uint8_t* id, int nbits, int* z_differs, int* a_inf,
             int* b_inf) {
  std::vector<int32_t> cw(54 * (T ? T : 1));
  for (uint32_t j = 0; j < T; ++j) {
    bool okd;
    td_store_g2p(cw.data() + j, T, proj_from_affine(g2_decode(commitments + 128 * j, okd)));
  }
  bool oki;
  uint32_t x[8], k[8];
  th_fr_words(fr_from_be(id, oki), x);
  const G2P b = g2_horner_lane(cw.data(), T, 0, T, x, nbits);
  // through the workspace, as the kernel reads it: canonical limbs
  std::vector<int32_t> r(54);
  td_store_g2p(r.data(), 1, b);
  const G2P key = td_load_g2p(r.data(), 1);
  bool ok;
  kc_share_words(share, k, ok);
  G2P a = kc_fixed_base_lane(tab, k);
  if (neg_a) a = proj_neg(a);
  *a_inf = fp2_is_zero(a.z) ? 1 : 0;
  *b_inf = fp2_is_zero(key.z) ? 1 : 0;
  *z_differs = fp2_is_zero(fp2_sub(a.z, key.z)) ? 0 : 1;
  if (neg_a) return (ok & proj_eq(a, key)) ? 1 : 0;
  return kc_key_check_lane(tab, k, ok, key) ? 1 : 0;
}

// bitmap ((N + 7) / 8 bytes) and status[g] as blsbn254_threshold_verify_key_shares_batch defines them (coff / goff: ng + 1
// offsets from 0); nbits must cover every usable id
void hs_kc_check(const int32_t* tab, const uint8_t* commitments, const uint32_t* coff, const uint8_t* ids, const uint8_t* shares, const uint32_t* goff, uint32_t ng, int nbits,
                 uint8_t* bitmap, uint8_t* status) {
  const size_t T = coff[ng], N = goff[ng];
  std::vector<int32_t> cw(54 * (T ? T : 1)), r(54 * (N ? N : 1));
  std::vector<uint8_t> c_ok(T ? T : 1), share_ok(N ? N : 1);
  std::vector<uint32_t> marks(ng, 0);
  for (size_t j = 0; j < T; ++j) {                                   // k_g2_load, k_g2_check
    bool okd;
    G2A p = g2_decode(commitments + 128 * j, okd);
    const bool good = okd & g2_on_curve(p);
    p.inf = p.inf | !good;
    td_store_g2p(cw.data() + j, T, proj_from_affine(p));
    c_ok[j] = (good && lane_g2_check(commitments + 128 * j)) ? 1 : 0;
  }
  for (size_t i = 0; i < N; ++i) {                                   // k_fr_decode, k_g2_poly_eval
    const uint32_t g = th_find_group(goff, ng, (uint32_t)i);
    bool o;
    const Fr v = fr_from_be(ids + 32 * i, o);
    const bool ok = o && !fr_is_zero(v);
    if (!ok) marks[g] |= TD_MARK_SCALAR;
    uint32_t k[8];
    th_fr_words(td_id_or_one(v, ok), k);
    td_store_g2p(r.data() + i, N, g2_horner_lane(cw.data(), T, coff[g], coff[g + 1], k, nbits));
  }
  for (size_t g = 0; g < ng; ++g) {                                  // k_td_finish
    uint8_t all = 1;
    for (uint32_t j = coff[g]; j < coff[g + 1]; ++j) all &= c_ok[j];
    if (!all) marks[g] |= TD_MARK_POINT;
    status[g] = (marks[g] & TD_MARK_SCALAR) ? 1 : (marks[g] & TD_MARK_POINT) ? 3 : 0;
  }
  for (size_t i = 0; i < N; ++i) {                                   // k_td_key_check
    uint32_t k[8];
    bool ok;
    kc_share_words(shares + 32 * i, k, ok);
    share_ok[i] = kc_key_check_lane(tab, k, ok, td_load_g2p(r.data() + i, N)) ? 1 : 0;
  }
  for (size_t b = 0; b < (N + 7) / 8; ++b) {                         // k_td_key_bits
    uint32_t v = 0;
    for (uint32_t j = 0; j < 8; ++j) {
      const size_t s = 8 * b + j;
      if (s < N && (share_ok[s] & 1) && marks[th_find_group(goff, ng, (uint32_t)s)] == 0) v |= 1u << j;
    }
    bitmap[b] = (uint8_t)v;
  }
}

}  // extern "C"
