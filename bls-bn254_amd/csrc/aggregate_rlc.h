// aggregate_rlc.h -- what ONE lane does in the aggregate verify over ragged groups by random linear combination
// (k_aggregate_rlc.hip, host_aggregate_rlc.hip).  For a range R of groups with weights r_g
//     prod_{g in R} [ e(sig_g, -G2gen) prod_i e(H_gi, pk_gi) ]^(r_g)
//       = e( sum_g r_g sig_g , -G2gen ) * prod_{distinct pk} e( sum_{(g,i): pk_gi = pk} r_g H_gi , pk )
// so one table-only Miller loop per distinct key (and one for the signatures) and ONE final exponentiation decide the range.
//   agr_sig_ok            the signature decodes, is on the curve and is not the identity (else the stand-in (1, 2))
//   agr_weight            r_g = a_g + b_g lambda: a_g, b_g = the first and the next 4 bytes, big-endian, of
//                         SHA-256(seed || "AGRLC" || g as 8 bytes LE || sig_g); (0, 0) becomes (1, 0).  The construction and the
//                         soundness argument of k_rlc2.hip: the 2^64 pairs give 2^64 distinct residues mod r
//   agr_mul_glv32         [a + b lambda] P by the 32-step joint double-and-add over {0, P, phi P, P + phi P}, P homogeneous;
//                         P + phi P = (beta^2 X, -Y, Z) needs no addition.  32 doublings and 32 additions whatever the bits
//   agr_store_point / agr_load_point   the layout k_g1_seg_sum reads: x, y, z limb-major
// aggregate_rlc_plan.h (included here) is the plain C++ of the host side.  tests/hostsim/aggregate_rlc_host.cpp compiles both for
// the host with -DBN_CHECK.  The lane functions are not a CPU fallback: nothing in the product's host path calls them.
#pragma once
#include "lane_ops.h"
#include "aggregate_rlc_plan.h"

namespace bn {

struct AgrWeight { uint32_t a, b; };

BN_FUNC bool agr_sig_ok(const uint8_t* sig, G1A& p) {
  bool okd;
  p = g1_decode(sig, okd);
  const bool ok = okd & !p.inf & g1_on_curve(p);
  p.x = fp_select(ok, p.x, fp_one()); p.y = fp_select(ok, p.y, fp_norm(fp_add(fp_one(), fp_one()))); p.inf = false;
  return ok;
}

BN_INL AgrWeight agr_weight_of_digest(const uint8_t* dg) {
  AgrWeight w;
  w.a = ((uint32_t)dg[0] << 24) | ((uint32_t)dg[1] << 16) | ((uint32_t)dg[2] << 8) | dg[3];
  w.b = ((uint32_t)dg[4] << 24) | ((uint32_t)dg[5] << 16) | ((uint32_t)dg[6] << 8) | dg[7];
  w.a = (w.a | w.b) ? w.a : 1u;                         // never the zero weight
  return w;
}
BN_FUNC AgrWeight agr_weight(const uint8_t* seed, uint64_t g, const uint8_t* sig) {
  const uint8_t tag[5] = {'A', 'G', 'R', 'L', 'C'};
  Sha256 s; sha256_init(s);
  sha256_update(s, seed, 32);
  sha256_update(s, tag, 5);
  for (int k = 0; k < 8; ++k) sha256_byte(s, (uint8_t)(g >> (8 * k)));
  sha256_update(s, sig, 64);
  uint8_t dg[32]; sha256_final(s, dg);
  return agr_weight_of_digest(dg);
}

// the entry of {0, P, phi P, P + phi P} named by the bit pair (a, b)
BN_INL G1P agr_pick4(bool a, bool b, const G1P& id, const G1P& p, const G1P& pf, const G1P& ps) {
  return proj_select(a, proj_select(b, ps, p), proj_select(b, pf, id));
}
BN_FUNC G1P agr_mul_glv32(const G1P& p, uint32_t a, uint32_t b) {
  BN_CTX;
  const G1P id = proj_identity<Fp>();
  // phi(X, Y, Z) = (beta X, Y, Z); P + phi(P) = -phi^2(P) = (beta^2 X, -Y, Z) with beta^2 = -1 - beta (lambda^2 + lambda + 1 = 0)
  const G1P pf = {fp_mul(p.x, fp_const(bnc::GLV_BETA)), p.y, p.z};
  const G1P ps = {fp_norm(fp_neg(fp_add(p.x, pf.x))), fp_norm(fp_neg(p.y)), p.z};
  G1P acc = id;
#pragma unroll 1
  for (int j = 31; j >= 0; --j) {
    acc = proj_dbl(acc);
    acc = proj_add(acc, agr_pick4((a >> j) & 1, (b >> j) & 1, id, p, pf, ps));
  }
  return acc;
}
// two points, each under its own weight, the chains interleaved step by step: each fills the multiply-add latency of the other
// (the two chains of k_rlc2_prep); every step computes what agr_mul_glv32 computes
BN_FUNC void agr_mul_glv32_x2(const G1P& p, const AgrWeight& wp, const G1P& q, const AgrWeight& wq, G1P& rp, G1P& rq) {
  BN_CTX;
  const G1P id = proj_identity<Fp>();
  const G1P pf = {fp_mul(p.x, fp_const(bnc::GLV_BETA)), p.y, p.z}, ps = {fp_norm(fp_neg(fp_add(p.x, pf.x))), fp_norm(fp_neg(p.y)), p.z};
  const G1P qf = {fp_mul(q.x, fp_const(bnc::GLV_BETA)), q.y, q.z}, qs = {fp_norm(fp_neg(fp_add(q.x, qf.x))), fp_norm(fp_neg(q.y)), q.z};
  G1P a1 = id, a2 = id;
#pragma unroll 1
  for (int j = 31; j >= 0; --j) {
    a1 = proj_dbl(a1); a2 = proj_dbl(a2);
    a1 = proj_add(a1, agr_pick4((wp.a >> j) & 1, (wp.b >> j) & 1, id, p, pf, ps));
    a2 = proj_add(a2, agr_pick4((wq.a >> j) & 1, (wq.b >> j) & 1, id, q, qf, qs));
  }
  rp = a1; rq = a2;
}

BN_FUNC void agr_store_point(int32_t* ws, size_t stride, const G1P& p) {
  store_fp(ws, stride, p.x); store_fp(ws + NL * stride, stride, p.y); store_fp(ws + 2 * NL * stride, stride, p.z);
}
BN_FUNC G1P agr_load_point(const int32_t* ws, size_t stride) {
  return {load_fp(ws, stride), load_fp(ws + NL * stride, stride), load_fp(ws + 2 * NL * stride, stride)};
}

}  // namespace bn
