// inflate.h -- compressed wire encodings to the uncompressed ones the pipelines read, one element per lane, with a per-element
// verdict instead of a per-batch error: g1_inflate (32 B -> 64 B) and g2_inflate (64 B -> 128 B) follow the rules of
// g1_decompress / g2_decompress (curve.h: flag = parity of y / sgn0(y), x == 0 is the identity whatever the flag, a coordinate
// >= p does not decode) and give the same bytes for every element that decodes.  An element that does not decode becomes THE
// MARKER, 0xFF in every output byte: g1_decode / g2_decode reject it (coordinate >= p), so every pipeline behind treats it as it
// treats any undecodable point and none of their kernels has to know where its input came from.  g1_inflate_point is g1_inflate
// for a lane that computes on with the point (the wire-format scans of keyset_agg.h): no bytes, no marker, a verdict.
//
// Both square roots come from fp_pow_pm3_4, the fixed addition chain for (p-3)/4 (fp29.h: 251 squarings + 52 products, uniform
// control flow, no exponent bit looked at), not from fp_pow's windows and not from an Fp2 ladder:
//   Fp:   y = a * a^((p-3)/4) = a^((p+1)/4); a is a square iff y^2 == a.
//   Fp2:  fp2_sqrt2 below, the "complex method" for u^2 = -1, p = 3 mod 4: two Fp chains and about 15 products where fp2_sqrt
//         (Algorithm 9 of eprint 2012/685) runs two 256-step square-and-always-multiply ladders in Fp2.
// Everything is selects: no branch on data, no data-dependent trip count, one instruction stream for every lane of a wave.
// tests/hostsim/inflate_host.cpp compiles this header for the host with -DBN_CHECK against Python integers and the oracle.
#pragma once
#include "curve.h"

namespace bn {

// A root of a = a0 + a1 u and whether a is a square.  With n = a0^2 + a1^2 (the norm) and s = sqrt(n) in Fp, a root x0 + x1 u
// satisfies x0^2 - x1^2 = a0 and x0^2 + x1^2 = +-s, so x0^2 = d = (a0 +- s) / 2 and x1 = a1 / (2 x0).  d == 0 with the plus sign
// means a1 == 0 and a0 = -s: the minus sign is taken instead (d = a0, or 0 for a == 0).  w = d^((p-3)/4) gives x0 = w d with
// x0^2 = d * d^((p-1)/2) = +-d:
//   x0^2 ==  d:  1 / x0 =  w, root = (x0, a1 w / 2)
//   x0^2 == -d:  d has no root in Fp but -d has (-1 is a non-residue): the root is u times the one above, (-a1 w / 2, x0),
//                with 1 / x0 = -w.  (a1 == 0 with a0 a non-residue lands here with h == 0: the root is x0 u.)
// The final comparison alone decides is_sq; it also rejects a non-residue n, for which s is no root of anything.
BN_FUNC Fp2 fp2_sqrt2(const Fp2& a_in, bool& is_sq) {
  BN_CTX;
  const Fp2 a = fp2_norm(a_in);
  const Fp half = fp_const(bnc::INV2);
  const Fp n = fp_dot2(a.c0, a.c0, a.c1, a.c1);
  const Fp s = fp_mul(n, fp_pow_pm3_4(n));
  const Fp sp = fp_norm(fp_add(a.c0, s)), sm = fp_norm(fp_sub(a.c0, s));
  const Fp d = fp_mul(fp_select(fp_is_zero(sp), sm, sp), half);
  const Fp w = fp_pow_pm3_4(d);
  const Fp x0 = fp_mul(w, d);
  const Fp h = fp_mul(fp_mul(a.c1, w), half);
  const bool plus = fp_eq(fp_sqr(x0), d);
  const Fp2 r = {fp_select(plus, x0, fp_norm(fp_neg(h))), fp_select(plus, h, x0)};
  is_sq = fp2_is_zero(fp2_sub(fp2_sqr(r), a));
  return r;
}

// 32 big-endian bytes of a (canonical), every byte OR-ed with the low byte of `fill`: fill = 0 writes the value, ~0 the marker
BN_INL void fp_to_be_fill(uint8_t* b, const Fp& a, uint32_t fill) {
  const Fp c = fp_from_mont(a);
  uint32_t w[8];
  limbs_to_words(w, c.l);
  BN_UNROLL for (int j = 0; j < 8; ++j) store_be32(b + 4 * (7 - j), w[j] | fill);
}

// in: 32 bytes (g1_compress).  out: the 64 bytes g1_decompress + g1_encode give, and true; or the marker, and false.
BN_FUNC bool g1_inflate(const uint8_t* in, uint8_t* out) {
  BN_CTX;
  uint8_t xb[32];
  for (int i = 0; i < 32; ++i) xb[i] = in[i];
  const int flag = xb[0] >> 7; xb[0] &= 0x7f;
  bool okx;
  const Fp x = fp_from_be(xb, okx);
  const bool inf = okx & fp_is_zero(x);
  const Fp rhs = fp_norm(fp_add(fp_mul(fp_sqr(x), x), fp_const(bnc::THREE)));
  const Fp y = fp_mul(rhs, fp_pow_pm3_4(rhs));
  const bool sq = fp_eq(fp_sqr(y), rhs);
  const bool flip = fp_sgn0(y) != flag;
  const Fp ys = fp_select(flip, fp_norm(fp_neg(y)), y);
  const bool ok = okx & (inf | sq);
  const uint32_t fill = ok ? 0u : ~0u;
  fp_to_be_fill(out, fp_select(inf, fp_zero(), x), fill);             // the identity is (0, 1), as g1_encode writes it
  fp_to_be_fill(out + 32, fp_select(inf, fp_one(), ys), fill);
  return ok;
}

// g1_inflate for a lane that goes on computing with the point instead of storing it: the same decoding, the same chain and the
// same selects, no bytes written.  The point comes back as th_point (threshold_batch.h) gives it on g1_inflate's bytes: x and y
// in the form fp_from_be leaves, the stand-in (1, 2) and ok = false where the encoding does not inflate, inf for x == 0.  The
// square test of the root IS the curve equation, so a caller has no second curve test to run.
BN_FUNC G1A g1_inflate_point(const uint8_t in[32], bool& ok) {
  BN_CTX;
  uint8_t xb[32];
  for (int i = 0; i < 32; ++i) xb[i] = in[i];
  const int flag = xb[0] >> 7; xb[0] &= 0x7f;
  bool okx;
  const Fp x = fp_from_be(xb, okx);
  const bool inf = okx & fp_is_zero(x);
  const Fp rhs = fp_norm(fp_add(fp_mul(fp_sqr(x), x), fp_const(bnc::THREE)));
  const Fp y = fp_mul(rhs, fp_pow_pm3_4(rhs));
  const bool sq = fp_eq(fp_sqr(y), rhs);
  const bool flip = fp_sgn0(y) != flag;
  const Fp ys = fp_select(flip, fp_norm(fp_neg(y)), y);
  ok = okx & (inf | sq);
  G1A p;
  p.x = fp_select(ok, x, fp_one());
  p.y = fp_select(ok, ys, fp_norm(fp_add(fp_one(), fp_one())));
  p.inf = inf;                                                         // (inf implies okx, so ok)
  return p;
}

// in: 64 bytes (g2_compress).  out: the 128 bytes g2_decompress + g2_encode give, and true; or the marker, and false.  The
// flag selects the root, so the bytes do not depend on which of the two roots fp2_sqrt2 (or fp2_sqrt) happens to find.
BN_FUNC bool g2_inflate(const uint8_t* in, uint8_t* out) {
  BN_CTX;
  uint8_t xb[32];
  for (int i = 0; i < 32; ++i) xb[i] = in[i];
  const int flag = xb[0] >> 7; xb[0] &= 0x7f;
  bool o0, o1, sq;
  Fp2 x;
  x.c1 = fp_from_be(xb, o0); x.c0 = fp_from_be(in + 32, o1);
  const bool inf = o0 & o1 & fp2_is_zero(x);
  const Fp2 rhs = fp2_norm(fp2_add(fp2_mul(fp2_sqr(x), x), fp2_const(bnc::B2)));
  const Fp2 y = fp2_sqrt2(rhs, sq);
  const bool flip = fp2_sgn0(y) != flag;
  const Fp2 ys = fp2_select(flip, fp2_norm(fp2_neg(y)), y);
  const bool ok = o0 & o1 & (inf | sq);
  const uint32_t fill = ok ? 0u : ~0u;
  const Fp2 ox = fp2_select(inf, fp2_zero(), x), oy = fp2_select(inf, fp2_one(), ys);
  fp_to_be_fill(out, ox.c1, fill); fp_to_be_fill(out + 32, ox.c0, fill);       // x.c1 | x.c0 | y.c1 | y.c0, as g2_encode
  fp_to_be_fill(out + 64, oy.c1, fill); fp_to_be_fill(out + 96, oy.c0, fill);
  return ok;
}

}  // namespace bn
