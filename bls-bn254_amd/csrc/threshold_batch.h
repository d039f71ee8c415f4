// threshold_batch.h -- what ONE lane does in the threshold combine over MANY groups (k_threshold_batch.hip,
// host_threshold_batch.hip): one lane per SHARE, group g owning the shares goff[g] .. goff[g + 1].
//     sigma_g = sum_{i in g} lambda_i sigma_i,   lambda_i = prod_{j in g, j != i} x_j / (x_j - x_i)
// (Scalar arithmetic scalar.rs:523-548, :216-219; Mul<Scalar> g1.rs:518-534, :821-841; Sum g1.rs:561-565 -- the same group
// element as the single-group pipeline of k_threshold.hip, hence the same bytes.)
//   th_find_group        the lane's group: the last g with goff[g] <= share (binary search, as the MSM bucket lanes find their bucket)
//   lagrange_seg_lane    the loop body of k_lagrange_partial over the lane's whole group, one inversion, GLV halves
//   g1_smul_glv_lane     [k1] P + [k2] phi(P) on ONE chain of 126 doublings: both 128-bit halves in signed odd 3-bit digits
//                        {+-1, +-3, +-5, +-7}, one table {P, 3P, 5P, 7P} for both (phi commutes with the group law, so the
//                        phi-side lookup is one multiplication of x by beta); the result stays homogeneous
// tests/hostsim/threshold_batch_host.cpp runs the same functions on the host with -DBN_CHECK (interval discipline) against
// the oracle.  They are not a CPU fallback: nothing in the product's host path calls them.
#pragma once
#include "lane_ops.h"
#include "fr29.h"
#include "glv.h"

namespace bn {

constexpr uint32_t TH_GID_BIG = 0x80000000u;     // gid word of a share whose group goes to the single-group pipeline
constexpr int TH_SMUL_WINDOWS = 43;              // 3-bit windows over 129 sign digits (a 128-bit half, made odd)
constexpr int TH_SMUL_TAB_LIMBS = 4 * 27;        // {P, 3P, 5P, 7P}, homogeneous, per lane

BN_INL void th_store_fr(int32_t* ws, size_t stride, const Fr& a) { for (int k = 0; k < NL; ++k) ws[(size_t)k * stride] = a.l[k]; }
BN_INL Fr th_load_fr(const int32_t* ws, size_t stride) { Fr r; for (int k = 0; k < NL; ++k) r.l[k] = ws[(size_t)k * stride]; return r; }

// a^(r-2) with 2-bit windows of the (public, wave-uniform) exponent: 254 squarings + at most 127 multiplications by a, a^2 or
// a^3, picked by a uniform select, so the three powers stay in registers (the 16-entry table of k_threshold.hip's fr_inv_w4 is
// indexed per iteration and lives in scratch)
BN_FUNC Fr fr_inv_w2(const Fr& a) {
  const Fr a2 = fr_mul(a, a), a3 = fr_mul(a2, a);
  Fr r = fr_const(bnc::FR_ONE);
#pragma unroll 1
  for (int w = 127; w >= 0; --w) {
    const uint64_t word = w >= 96 ? bnc::EXP_RM2[3] : w >= 64 ? bnc::EXP_RM2[2] : w >= 32 ? bnc::EXP_RM2[1] : bnc::EXP_RM2[0];
    const int d = (int)((word >> ((w & 31) * 2)) & 3);
    r = fr_mul(r, r); r = fr_mul(r, r);
    if (d) r = fr_mul(r, fr_select(d == 1, a, fr_select(d == 2, a2, a3)));
  }
  return r;
}

// the last g in [0, ng) with goff[g] <= s; the caller guarantees goff[0] <= s < goff[ng] (empty groups are stepped over:
// of several equal offsets the last one starts the group that holds s)
BN_INL uint32_t th_find_group(const uint32_t* goff, uint32_t ng, uint32_t s) {
  uint32_t lo = 0, hi = ng - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (goff[mid] <= s) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Lane i of a launch of m shares (x_ws: their decoded ids, limb-major, stride m; id_ok: bit 0 = decodes and non-zero); its
// group is the shares [a, b) of the launch.  Returns lambda_i in Montgomery form; bad = the lane's own id is unusable or
// some OTHER id of the group equals it (ids of other groups are never looked at).
BN_FUNC Fr lagrange_seg_lane(const int32_t* x_ws, const uint8_t* id_ok, size_t m, uint32_t i, uint32_t a, uint32_t b, bool& bad) {
  const Fr xi = th_load_fr(x_ws + i, m);
  Fr num = fr_const(bnc::FR_ONE), den = num;
  const Fr one = num;
  bool d = false;
#pragma unroll 1
  for (uint32_t j = a; j < b; ++j) {
    const Fr xj = th_load_fr(x_ws + j, m);
    const Fr df = fr_sub(xj, xi);
    const bool self = j == i;
    d |= !self & fr_is_zero(df);
    num = fr_mul(num, fr_select(self, one, xj));
    den = fr_mul(den, fr_select(self, one, df));
  }
  bad = d | !(id_ok[i] & 1);
  return fr_mul(num, fr_inv_w2(den));
}
// lambda (Montgomery) -> canonical little-endian words
BN_INL void th_fr_words(const Fr& lam, uint32_t w[8]) {
  Fr one; for (int k = 0; k < NL; ++k) one.l[k] = k == 0;
  const Fr c = fr_mul(lam, one);                            // out of Montgomery form, canonical
  limbs_to_words(w, c.l);
}

// window i (0 .. 42) of the 128-bit magnitude k read as 129 sign digits s_j = 2 bit_(j+1) - 1 (s_128 = +1): for ODD k,
// k = sum_j s_j 2^j, so the window's digit s_3i + 2 s_(3i+1) + 4 s_(3i+2) = 2 v - 7 with v = bits 3i+1 .. 3i+3 of k (bit 129
// read as 1).  Bit 0 is never read: an even k is recoded as k + 1 and the caller takes one P off at the end.
BN_INL uint32_t th_window_bits(const uint32_t* k, int i) {
  const int pos = 3 * i + 1, w = pos >> 5, o = pos & 31;
  uint32_t lo = 0, hi = 0;
  BN_UNROLL for (int j = 0; j < 4; ++j) { lo = j == w ? k[j] : lo; hi = j == w + 1 ? k[j] : hi; }
  const uint64_t v = ((uint64_t)hi << 32) | lo;
  uint32_t r = (uint32_t)(v >> o) & 7u;
  return i == TH_SMUL_WINDOWS - 1 ? ((r & 1u) | 4u) : r;     // bits 127, (128 = 0), (129 = 1)
}
// the table entry for window bits v with the half's sign folded in: +-(2e + 1) P, or its image under phi
BN_INL G1P th_tab_entry(const Ws& tab, uint32_t v, bool half_neg, bool phi) {
  const uint32_t e = v >= 4 ? v - 4 : 3 - v;
  const bool neg = (v < 4) != half_neg;
  const Ws t = ws_at(tab, 27 * e);
  G1P p = {fp_load_mem(t), fp_load_mem(ws_at(t, 9)), fp_load_mem(ws_at(t, 18))};
  if (phi) p.x = fp_mul(p.x, fp_const(bnc::GLV_BETA));
  p.y = fp_select(neg, fp_norm(fp_neg(p.y)), p.y);
  return p;
}
BN_INL void th_tab_store(const Ws& tab, int e, const G1P& p) {
  const Ws t = ws_at(tab, 27 * e);
  fp_store_mem(t, p.x); fp_store_mem(ws_at(t, 9), p.y); fp_store_mem(ws_at(t, 18), p.z);
}
// [k1] P + [k2] phi(P) for the GLV halves g of a scalar (glv_split); P affine and ON THE CURVE (or the identity).  tab: the
// lane's own column of TH_SMUL_TAB_LIMBS limbs (LDS on the device).  126 doublings + 1, 84 + 6 complete additions.
BN_FUNC G1P g1_smul_glv_lane(const G1A& pa, const GlvSplit& g, const Ws& tab) {
  BN_CTX;
  const G1P p = proj_from_affine(pa);
  {
    const G1P p2 = proj_dbl(p);
    G1P q = p;
    th_tab_store(tab, 0, q);
    for (int e = 1; e < 4; ++e) { q = proj_add(q, p2); th_tab_store(tab, e, q); }
  }
  BN_MEM_FENCE;
  G1P acc = proj_add(th_tab_entry(tab, th_window_bits(g.k1, TH_SMUL_WINDOWS - 1), g.neg1, false),
                     th_tab_entry(tab, th_window_bits(g.k2, TH_SMUL_WINDOWS - 1), g.neg2, true));
#pragma unroll 1
  for (int i = TH_SMUL_WINDOWS - 2; i >= 0; --i) {
    acc = proj_dbl(proj_dbl(proj_dbl(acc)));
    acc = proj_add(acc, th_tab_entry(tab, th_window_bits(g.k1, i), g.neg1, false));
    acc = proj_add(acc, th_tab_entry(tab, th_window_bits(g.k2, i), g.neg2, true));
  }
  // even halves were recoded as k + 1: take that P (with the half's sign) off again
  const G1P id = proj_identity<Fp>();
  const G1P c1 = th_tab_entry(tab, 3, g.neg1, false), c2 = th_tab_entry(tab, 3, g.neg2, true);   // v = 3: -P, sign folded
  acc = proj_add(acc, proj_select((g.k1[0] & 1u) == 0, c1, id));
  acc = proj_add(acc, proj_select((g.k2[0] & 1u) == 0, c2, id));
  return acc;
}
// a share's point for the multiplication: decodes AND satisfies the curve equation (the identity included), else the
// stand-in (1, 2) so that no lane computes on garbage; ok tells which
BN_INL G1A th_point(const uint8_t* g1, bool& ok) {
  bool okd;
  G1A p = g1_decode(g1, okd);
  ok = okd & g1_on_curve(p);
  G1A s; s.x = fp_one(); s.y = fp_norm(fp_add(fp_one(), fp_one())); s.inf = false;
  p.x = fp_select(ok, p.x, s.x); p.y = fp_select(ok, p.y, s.y); p.inf = ok & p.inf;
  return p;
}

}  // namespace bn
