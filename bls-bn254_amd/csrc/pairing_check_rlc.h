// pairing_check_rlc.h -- what ONE lane does in the pairing-product checks over ragged groups by random linear combination
// (k_pairing_check_rlc.hip, host_pairing_check_rlc.hip).  For a range R of equations with weights r_g
//     prod_{g in R} [ prod_j e(P_gj, Q_gj) ]^(r_g)  =  prod_{distinct Q} e( sum_{(g,j): Q_gj = Q} r_g P_gj , Q )
// so one table-only Miller loop per distinct Q and ONE final exponentiation decide the range.  Weighing P is the r_g-th power
// only for a Q in the r-torsion (e(P, Q)^r = e(P, [r] Q)): that is why a pair is OK only with such a Q.
//   pcr_pair              the pair's byte: PCR_OK when P decodes and is on the curve (identity allowed) and Q is the identity by its
//                         encoding (x = 0) or valid by the key preparation of the DISTINCT Q (key_ok: decodes, on the curve, in
//                         the r-torsion) -- k_pair_ok's predicate without a torsion test per pair; PCR_SKIP when P or Q is
//                         the identity by its encoding.  The decoded P, or the stand-in (1, 2) for a pair that is skipped or not OK
//   pcr_eligible          an equation's byte: the AND of its pairs' OK bits
//   pcr_weight            r_g = a_g + b_g lambda: a_g, b_g from SHA-256(seed || "PCRLC" || g as 8 bytes LE) through
//                         agr_weight_of_digest (aggregate_rlc.h: big-endian halves, (0, 0) becomes (1, 0), and its soundness argument)
//   pcr_mul_glv32         [a + b lambda] P by the 32-step joint double-and-add over {0, P, phi P, P + phi P} for an AFFINE P: the
//                         three entries are affine, so every addition is proj_add_mixed (11 products for 12) and the entry 0
//                         keeps the doubled value by selection.  32 doublings and 32 mixed additions whatever the bits
//   pcr_mul_glv32_x2      two such chains interleaved step by step, as agr_mul_glv32_x2
//   pcr_store_affine / pcr_load_affine   x, y limb-major: what k_pcr_pairs leaves for k_pcr_weigh (no point is decoded twice)
// The weighted points leave in agr_store_point's layout, which k_g1_seg_sum reads.  tests/hostsim/pairing_check_rlc_host.cpp
// compiles this for the host with -DBN_CHECK.  The lane functions are not a CPU fallback: nothing in the product's host path calls them.
#pragma once
#include "aggregate_rlc.h"
#include "pairing_check_rlc_plan.h"

namespace bn {

enum : uint8_t { PCR_OK = 1, PCR_SKIP = 2 };

// Q is the identity by its encoding: x.c1 = x.c0 = 0, both canonical (g2_decode's `inf`, without reading y)
BN_INL bool pcr_q_identity(const uint8_t* g2) {
  bool o0, o1;
  const Fp c1 = fp_from_be(g2, o0), c0 = fp_from_be(g2 + 32, o1);
  return o0 & o1 & fp_is_zero(c1) & fp_is_zero(c0);
}
BN_FUNC uint8_t pcr_pair(const uint8_t* g1, const uint8_t* g2, uint8_t key_ok, G1A& p) {
  bool ok1;
  p = g1_decode(g1, ok1);
  const bool q_inf = pcr_q_identity(g2);
  const bool ok = ok1 & g1_on_curve(p) & (q_inf | (key_ok != 0));
  const bool skip = p.inf | q_inf;
  const bool use = ok & !skip;
  p.x = fp_select(use, p.x, fp_one()); p.y = fp_select(use, p.y, fp_norm(fp_add(fp_one(), fp_one()))); p.inf = false;
  return (uint8_t)((ok ? PCR_OK : 0) | (skip ? PCR_SKIP : 0));
}

// an equation is eligible when all its pairs flag[p0 .. p1) are OK (an empty one is)
BN_INL bool pcr_eligible(const uint8_t* flag, uint32_t p0, uint32_t p1) {
  uint8_t ok = PCR_OK;
#pragma unroll 1
  for (uint32_t i = p0; i < p1; ++i) ok &= flag[i];
  return ok != 0;
}

BN_FUNC AgrWeight pcr_weight(const uint8_t* seed, uint64_t g) {
  const uint8_t tag[5] = {'P', 'C', 'R', 'L', 'C'};
  Sha256 s; sha256_init(s);
  sha256_update(s, seed, 32);
  sha256_update(s, tag, 5);
  for (int k = 0; k < 8; ++k) sha256_byte(s, (uint8_t)(g >> (8 * k)));
  uint8_t dg[32]; sha256_final(s, dg);
  return agr_weight_of_digest(dg);
}

// P, phi P = (beta x, y) and P + phi P = -phi^2 P = (beta^2 x, -y) share two y values: three x and two y name the three entries
struct PcrTab { Fp x, xf, xs, y, ny; };
BN_INL PcrTab pcr_tab(const G1A& p) {
  BN_CTX;
  PcrTab t;
  t.x = p.x; t.xf = fp_mul(p.x, fp_const(bnc::GLV_BETA)); t.xs = fp_norm(fp_neg(fp_add(p.x, t.xf)));
  t.y = p.y; t.ny = fp_norm(fp_neg(p.y));
  return t;
}
// the entry named by the bit pair (a, b); (0, 0) names P, and the caller keeps its accumulator instead
BN_INL G1A pcr_pick3(bool a, bool b, const PcrTab& t) {
  return {fp_select(a, fp_select(b, t.xs, t.x), fp_select(b, t.xf, t.x)), fp_select(a & b, t.ny, t.y), false};
}
BN_INL G1P pcr_step(const G1P& acc, bool a, bool b, const PcrTab& t) {
  const G1P d = proj_dbl(acc);
  return proj_select(a | b, proj_add_mixed(d, pcr_pick3(a, b, t)), d);
}
BN_FUNC G1P pcr_mul_glv32(const G1A& p, uint32_t a, uint32_t b) {
  BN_CTX;
  const PcrTab t = pcr_tab(p);
  G1P acc = proj_identity<Fp>();
#pragma unroll 1
  for (int j = 31; j >= 0; --j) acc = pcr_step(acc, (a >> j) & 1, (b >> j) & 1, t);
  return acc;
}
BN_FUNC void pcr_mul_glv32_x2(const G1A& p, const AgrWeight& wp, const G1A& q, const AgrWeight& wq, G1P& rp, G1P& rq) {
  BN_CTX;
  const PcrTab tp = pcr_tab(p), tq = pcr_tab(q);
  G1P a1 = proj_identity<Fp>(), a2 = a1;
#pragma unroll 1
  for (int j = 31; j >= 0; --j) {
    const G1P d1 = proj_dbl(a1), d2 = proj_dbl(a2);
    const bool pa = (wp.a >> j) & 1, pb = (wp.b >> j) & 1, qa = (wq.a >> j) & 1, qb = (wq.b >> j) & 1;
    a1 = proj_select(pa | pb, proj_add_mixed(d1, pcr_pick3(pa, pb, tp)), d1);
    a2 = proj_select(qa | qb, proj_add_mixed(d2, pcr_pick3(qa, qb, tq)), d2);
  }
  rp = a1; rq = a2;
}

BN_FUNC void pcr_store_affine(int32_t* ws, size_t stride, const G1A& p) { store_fp(ws, stride, p.x); store_fp(ws + NL * stride, stride, p.y); }
BN_FUNC G1A pcr_load_affine(const int32_t* ws, size_t stride) { return {load_fp(ws, stride), load_fp(ws + NL * stride, stride), false}; }

}  // namespace bn
