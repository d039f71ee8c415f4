// threshold_deal_host.cpp -- the lane functions of csrc/threshold_deal.h (key shares and their public keys over many groups)
// compiled for the host with -DBN_CHECK (every field operation asserts the lazy-limb interval discipline), for
// tests/test_threshold_deal_host.py: the Horner evaluation in Fr and "in the exponent" of G2, run lane by lane as the kernels
// of k_threshold_deal.hip index them, with the marks and statuses of the finish kernels.  TEST TOOL ONLY.
#include "../../bls-bn254_amd/csrc/threshold_deal.h"
#include <vector>

using namespace bn;

namespace {
// k_fr_decode over N ids: Montgomery limbs (stride N), ok = decodes and non-zero
void decode_ids(const uint8_t* ids, size_t N, std::vector<int32_t>& x, std::vector<uint8_t>& ok) {
  x.assign(9 * (N ? N : 1), 0); ok.assign(N ? N : 1, 0);
  for (size_t i = 0; i < N; ++i) {
    bool o;
    const Fr v = fr_from_be(ids + 32 * i, o);
    th_store_fr(x.data() + i, N, v);
    ok[i] = (o && !fr_is_zero(v)) ? 1 : 0;
  }
}
// k_td_finish: the marks the lanes left and the validity bytes of the group's coefficients / commitments -> mark word, status
void finish(std::vector<uint32_t>& marks, const uint32_t* coff, const std::vector<uint8_t>& ok, uint32_t mark, uint8_t* status) {
  for (size_t g = 0; g < marks.size(); ++g) {
    uint8_t all = 1;
    for (uint32_t j = coff[g]; j < coff[g + 1]; ++j) all &= ok[j];
    if (!all) marks[g] |= mark;
    status[g] = (marks[g] & TD_MARK_SCALAR) ? 1 : (marks[g] & TD_MARK_POINT) ? 3 : 0;
  }
}
}  // namespace

extern "C" {

// out[32 i ..] and status[g] as blsbn254_fr_poly_eval_batch defines them (coff / goff: ng + 1 offsets from 0)
void hs_td_fr_eval(const uint8_t* coeffs, const uint32_t* coff, const uint8_t* ids, const uint32_t* goff, uint32_t ng, uint8_t* out, uint8_t* status) {
  const size_t T = coff[ng], N = goff[ng];
  std::vector<int32_t> cf(9 * (T ? T : 1)), r(9 * (N ? N : 1)), x;
  std::vector<uint8_t> ok, cf_ok(T ? T : 1);
  std::vector<uint32_t> marks(ng, 0);
  for (size_t j = 0; j < T; ++j) {                                   // k_fr_coef_decode
    bool o;
    th_store_fr(cf.data() + j, T, fr_from_be(coeffs + 32 * j, o));
    cf_ok[j] = o ? 1 : 0;
  }
  decode_ids(ids, N, x, ok);
  for (size_t i = 0; i < N; ++i) {                                   // k_fr_poly_eval
    const uint32_t g = th_find_group(goff, ng, (uint32_t)i);
    if (!ok[i]) marks[g] |= TD_MARK_SCALAR;
    th_store_fr(r.data() + i, N, fr_horner_lane(cf.data(), T, coff[g], coff[g + 1], td_id_or_one(th_load_fr(x.data() + i, N), ok[i])));
  }
  finish(marks, coff, cf_ok, TD_MARK_SCALAR, status);
  for (size_t i = 0; i < N; ++i)                                     // k_td_fr_encode
    fr_to_be(out + 32 * i, fr_select(marks[th_find_group(goff, ng, (uint32_t)i)] != 0, Fr{}, th_load_fr(r.data() + i, N)));
}

// out[128 i ..] and status[g] as blsbn254_g2_poly_eval_batch defines them, with the launch's bit count given by the caller
// (it must cover every usable id)
void hs_td_g2_eval(const uint8_t* commitments, const uint32_t* coff, const uint8_t* ids, const uint32_t* goff, uint32_t ng, int nbits, uint8_t* out,
                   uint8_t* status) {
  const size_t T = coff[ng], N = goff[ng];
  std::vector<int32_t> cw(54 * (T ? T : 1)), r(54 * (N ? N : 1)), x;
  std::vector<uint8_t> ok, c_ok(T ? T : 1);
  std::vector<uint32_t> marks(ng, 0);
  for (size_t j = 0; j < T; ++j) {                                   // k_g2_load, k_g2_check
    bool okd;
    G2A p = g2_decode(commitments + 128 * j, okd);
    const bool good = okd & g2_on_curve(p);
    p.inf = p.inf | !good;
    td_store_g2p(cw.data() + j, T, proj_from_affine(p));
    c_ok[j] = (good && lane_g2_check(commitments + 128 * j)) ? 1 : 0;
  }
  decode_ids(ids, N, x, ok);
  for (size_t i = 0; i < N; ++i) {                                   // k_g2_poly_eval
    const uint32_t g = th_find_group(goff, ng, (uint32_t)i);
    if (!ok[i]) marks[g] |= TD_MARK_SCALAR;
    uint32_t k[8];
    th_fr_words(td_id_or_one(th_load_fr(x.data() + i, N), ok[i]), k);
    td_store_g2p(r.data() + i, N, g2_horner_lane(cw.data(), T, coff[g], coff[g + 1], k, nbits));
  }
  finish(marks, coff, c_ok, TD_MARK_POINT, status);
  for (size_t i = 0; i < N; ++i)                                     // k_td_g2_encode
    g2_encode(out + 128 * i, g2_to_affine(proj_select(marks[th_find_group(goff, ng, (uint32_t)i)] != 0, proj_identity<Fp2>(), td_load_g2p(r.data() + i, N))));
}

}  // extern "C"
