// msm.h -- multi-scalar multiplication out = sum_i [k_i] P_i by the bucket (Pippenger) method, field-generic (F = Fp: G1,
// F = Fp2: G2), as curve.h is.  (LinearCombination for G1Projective g1.rs:559 / G2Projective g2.rs:577, n-term form; the
// value is Mul<Scalar> g1.rs:518-534 + Sum g1.rs:561-565, so the output bytes are the reference's.)
//
//   recode   G1: k = k1 + k2 lambda (glv.h), |k1|, |k2| <= 2^127, the signs folded into the point (-P = (x, -y)) and
//            phi(P) = (beta x, y) stored as a second row; G2: the full 254-bit scalar (psi is only an endomorphism on the
//            r-torsion, and the G2 entry points accept points outside it).  Signed c-bit digits d in [-2^(c-1), 2^(c-1)] over
//            ceil((bits + 1) / c) windows.  Digit d != 0 of a non-identity point = one bucket entry: key (window, |d| - 1),
//            value (row << 1 | sign).
//   sort     counting sort of the entries by key, per window (k_kd_msm_hist / k_scan_excl / k_kd_msm_scatter).
//   buckets  levels of chunk sums: at level l a lane adds at most L = 2^MSM_LG_CHUNK inputs of ONE bucket (level 0: affine
//            points gathered from the limb-major point rows, mixed additions; later levels: the previous level's partial
//            sums).  Level l's outputs of bucket b live at slots off_l(b) = (start_b >> (lgL (l + 1))) + b, ..., a layout
//            that needs no scan (the ranges of consecutive buckets never overlap); the last level writes bucket b at b.
//            A bucket of a million entries (every scalar equal) is summed by a tree of chunk lanes, never by one lane.
//   reduce   per window sum_j j S_j by running sums over G segments of the bucket range: segment g gives
//            R_g + (g Lseg) T_g with R_g, T_g its running sums.
//   final    the segments of each window summed in LDS, the windows combined by Horner (c doublings each), affine bytes.
// Every function below is what ONE lane does; the kernels (k_msm_bucket.hip) only index.  tests/hostsim/msm_host.cpp runs the
// same functions on the host with -DBN_CHECK (interval discipline) against the oracle.
#pragma once
#include "lane_ops.h"
#include "glv.h"

namespace bn {

constexpr uint32_t MSM_NO_KEY = 0xffffffffu;     // zero digit or identity point: no bucket entry
constexpr int MSM_LG_CHUNK = 5;                  // L = 32 entries per lane and level of the bucket sums
constexpr int MSM_MAX_SEGS = 256;                // segments per window of the bucket reduction (one workgroup sums them)

BN_INL int msm_windows(int bits, int c) { return (bits + c) / c; }      // ceil((bits + 1) / c): room for the last carry

// ------------------------------------------------------------------ field-generic limb-major storage
template <class F> struct FLimbs;
template <> struct FLimbs<Fp> { static constexpr int n = NL; };
template <> struct FLimbs<Fp2> { static constexpr int n = 2 * NL; };
BN_INL void msm_store(int32_t* ws, size_t st, const Fp& a) { store_fp(ws, st, a); }
BN_INL void msm_store(int32_t* ws, size_t st, const Fp2& a) { store_fp(ws, st, a.c0); store_fp(ws + NL * st, st, a.c1); }
BN_INL void msm_load(const int32_t* ws, size_t st, Fp& a) { a = load_fp(ws, st); }
BN_INL void msm_load(const int32_t* ws, size_t st, Fp2& a) { a.c0 = load_fp(ws, st); a.c1 = load_fp(ws + NL * st, st); }
// projective point: x, y, z one after the other (3 FLimbs rows)
template <class F> BN_INL void msm_store_p(int32_t* ws, size_t st, const Proj<F>& p) {
  constexpr int K = FLimbs<F>::n;
  msm_store(ws, st, p.x); msm_store(ws + K * st, st, p.y); msm_store(ws + 2 * K * st, st, p.z);
}
template <class F> BN_INL Proj<F> msm_load_p(const int32_t* ws, size_t st) {
  constexpr int K = FLimbs<F>::n;
  Proj<F> p;
  msm_load(ws, st, p.x); msm_load(ws + K * st, st, p.y); msm_load(ws + 2 * K * st, st, p.z);
  return p;
}

// ------------------------------------------------------------------ scalar recoding
// bits [pos, pos + c) of the little-endian words k[0..NW), c <= 16; the words are picked by compare-and-select, so a lane's
// scalar stays in registers
template <int NW> BN_INL uint32_t msm_bits(const uint32_t* k, int pos, int c) {
  const int w = pos >> 5, o = pos & 31;
  uint32_t lo = 0, hi = 0;
  BN_UNROLL for (int j = 0; j < NW; ++j) { lo = j == w ? k[j] : lo; hi = j == w + 1 ? k[j] : hi; }
  const uint64_t v = ((uint64_t)hi << 32) | lo;
  return (uint32_t)(v >> o) & ((1u << c) - 1u);
}
// next signed digit: v = window bits + carry; v > 2^(c-1) becomes v - 2^c with a carry into the next window.
// d in [-2^(c-1) + 1, 2^(c-1)]
BN_INL int32_t msm_digit(uint32_t bits, int c, uint32_t& carry) {
  const uint32_t v = bits + carry, half = 1u << (c - 1);
  carry = v > half ? 1u : 0u;
  return (int32_t)v - (int32_t)(carry << c);
}
// the W = msm_windows(bits, c) entries of one (point row, scalar) pair: window w's key / value at key[w * wstride].
// neg: the scalar's sign (G1 GLV halves); live = false (identity or invalid point) writes no entry.
template <int NW> BN_INL void msm_recode_store(const uint32_t* k, int c, int W, bool neg, bool live, uint32_t row,
                                               uint32_t* key, uint32_t* val, size_t wstride) {
  uint32_t carry = 0;
#pragma unroll 1
  for (int w = 0; w < W; ++w) {
    const int32_t d = msm_digit(msm_bits<NW>(k, w * c, c), c, carry);
    const bool has = live & (d != 0);
    key[(size_t)w * wstride] = has ? (uint32_t)((d < 0 ? -d : d) - 1) : MSM_NO_KEY;
    val[(size_t)w * wstride] = (row << 1) | ((d < 0) != neg ? 1u : 0u);
  }
}
// 32 bytes big-endian -> 8 little-endian words
BN_INL void msm_scalar_words(const uint8_t* be, uint32_t w[8]) {
  BN_UNROLL for (int j = 0; j < 8; ++j)
    w[j] = ((uint32_t)be[28 - 4 * j] << 24) | ((uint32_t)be[29 - 4 * j] << 16) | ((uint32_t)be[30 - 4 * j] << 8) | be[31 - 4 * j];
}

// ------------------------------------------------------------------ group law
// complete mixed addition P + (x2, y2), Z2 = 1: RCB 2015/1060 Alg 8 with a = 0 (11 M + 2 m_3b).  The affine operand must not be
// the identity (an identity point makes no bucket entry); P may be.  Cross terms formed subtractively as in proj_add.
template <class F> BN_FUNC Proj<F> proj_madd(const Proj<F>& a, const F& x2, const F& y2) {
  BN_CTX;
  F t0 = f_mul(a.x, x2), t1 = f_mul(a.y, y2);
  F m3 = f_mul(f_sub(a.x, a.y), f_sub(x2, y2));
  F t3 = f_lc3<1, 1, -1>(t0, t1, m3);              // X1Y2 + X2Y1
  F t4 = f_norm(f_add(f_mul(y2, a.z), a.y));       // Y1 + Y2Z1
  F y3 = f_norm(f_add(f_mul(x2, a.z), a.x));       // X1 + X2Z1
  F t0_3 = f_lc2<3, 0>(t0, t0);                    // 3 X1X2
  F bt2 = f_mul_b3(a.z);
  F z3 = f_norm(f_add(t1, bt2));
  F t1m = f_norm(f_sub(t1, bt2));
  F by3 = f_mul_b3(y3);
  F x3 = f_norm(f_sub(f_mul(t3, t1m), f_mul(t4, by3)));
  F yy = f_norm(f_add(f_mul(t1m, z3), f_mul(by3, t0_3)));
  F zz = f_norm(f_add(f_mul(z3, t4), f_mul(t0_3, t3)));
  return {x3, yy, zz};
}
// [m] P for a small public m < 2^nbits (the segment offsets of the reduction): double and add, complete formulas
template <class F> BN_FUNC Proj<F> proj_mul_small(const Proj<F>& p, uint32_t m, int nbits) {
  BN_CTX;
  Proj<F> acc = proj_identity<F>();
#pragma unroll 1
  for (int b = nbits - 1; b >= 0; --b) {
    acc = proj_dbl(acc);
    if ((m >> b) & 1u) acc = proj_add(acc, p);
  }
  return acc;
}

// ------------------------------------------------------------------ bucket sums
// start of bucket b in the sorted entries (run_end = the scatter cursors after the sort: one past the bucket's last entry)
BN_INL uint32_t msm_bucket_start(const uint32_t* hist, const uint32_t* run_end, uint32_t b) { return run_end[b] - hist[b]; }
// inputs of bucket b at level l: h_b entries (l = 0) or ceil(h_b / L^l) partial sums
BN_INL uint32_t msm_level_inputs(uint32_t h, int level) {
  const int sh = MSM_LG_CHUNK * level;
  return (uint32_t)(((uint64_t)h + ((1ull << sh) - 1)) >> sh);
}
BN_INL uint32_t msm_level_off(uint32_t start, uint32_t b, int level) { return (uint32_t)(start >> (MSM_LG_CHUNK * (level + 1))) + b; }

// One lane of level `level`.  final_level: lane = bucket b, output slot b, all of its inputs.  Otherwise lane = output slot s:
// the bucket is the last b with off_level(b) <= s (binary search over the u buckets), chunk j = s - off_level(b).
// Level 0 reads entries sorted[start_b ..] and the affine rows pts (x then y, FLimbs each, stride rows); level l > 0 reads
// the previous level's partials in_ws (stride in_st) at off_{l-1}(b).  Slots of no chunk are left unwritten (never read).
template <class F> BN_FUNC void msm_bucket_lane(uint32_t s, int level, bool final_level, const uint32_t* hist, const uint32_t* run_end, uint32_t u,
                                                const uint32_t* sorted, const int32_t* pts, size_t rows, const int32_t* in_ws, size_t in_st,
                                                int32_t* out_ws, size_t out_st) {
  constexpr int K = FLimbs<F>::n;
  constexpr uint32_t L = 1u << MSM_LG_CHUNK;
  uint32_t b, j;
  if (final_level) {
    if (s >= u) return;
    b = s; j = 0;
  } else {
    uint32_t lo = 0, hi = u - 1;                   // off_level is strictly increasing in b, off_level(0) = start_0 >> .. = 0
    while (lo < hi) {
      const uint32_t mid = (lo + hi + 1) >> 1;
      if (msm_level_off(msm_bucket_start(hist, run_end, mid), mid, level) <= s) lo = mid; else hi = mid - 1;
    }
    b = lo;
    j = s - msm_level_off(msm_bucket_start(hist, run_end, b), b, level);
  }
  const uint32_t h = hist[b], start = msm_bucket_start(hist, run_end, b);
  const uint32_t n_in = msm_level_inputs(h, level);
  if (!final_level && j >= ((n_in + L - 1) >> MSM_LG_CHUNK)) return;
  const uint32_t first = final_level ? 0 : j * L;
  const uint32_t last = final_level ? n_in : (first + L < n_in ? first + L : n_in);
  Proj<F> acc = proj_identity<F>();
  if (level == 0) {
#pragma unroll 1
    for (uint32_t t = first; t < last; ++t) {
      const uint32_t v = sorted[start + t];
      const size_t row = v >> 1;
      F x, y;
      msm_load(pts + row, rows, x); msm_load(pts + K * rows + row, rows, y);
      y = f_select((v & 1u) != 0, f_norm(f_neg(y)), y);
      acc = proj_madd(acc, x, y);
    }
  } else {
    const uint32_t base = msm_level_off(start, b, level - 1);
#pragma unroll 1
    for (uint32_t t = first; t < last; ++t) acc = proj_add(acc, msm_load_p<F>(in_ws + base + t, in_st));
  }
  msm_store_p(out_ws + (final_level ? b : s), out_st, acc);
}

// ------------------------------------------------------------------ bucket reduction
// Lane (w, g): buckets idx in [g Lseg, (g + 1) Lseg) of window w hold the sums S_idx of digit magnitude idx + 1.  Running sums
// from the top, T = sum S, R = sum (idx - g Lseg + 1) S; the segment's share of sum_j j S_j is R + (g Lseg) T.
// bsum: the last level's bucket sums (stride u), seg_out: W x G points (stride W G).
template <class F> BN_FUNC void msm_reduce_lane(uint32_t w, uint32_t g, uint32_t B, uint32_t G, int c, const int32_t* bsum, size_t u,
                                                int32_t* seg_out, size_t seg_st) {
  const uint32_t lseg = B / G, lo = g * lseg;
  Proj<F> T = proj_identity<F>(), R = proj_identity<F>();
#pragma unroll 1
  for (uint32_t k = lseg; k-- > 0;) {
    T = proj_add(T, msm_load_p<F>(bsum + (size_t)w * B + lo + k, u));    // the last level wrote every bucket (empty: identity)
    R = proj_add(R, T);
  }
  R = proj_add(R, proj_mul_small(T, lo, c - 1));
  msm_store_p(seg_out + (size_t)w * G + g, seg_st, R);
}

}  // namespace bn
