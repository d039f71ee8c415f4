// msm_host.cpp -- the multi-scalar multiplication lane functions of csrc/msm.h compiled for the host with -DBN_CHECK (every field
// operation asserts the lazy-limb interval discipline), for tests/test_msm_host.py: digit recoding, the complete mixed addition,
// and the whole recode -> sort -> bucket levels -> reduce -> Horner pipeline run lane by lane.  TEST TOOL ONLY.
#include "../../bls-bn254_amd/csrc/msm.h"
#include <vector>

using namespace bn;

extern "C" {

// digits of one scalar (32 B big-endian): half = -1 the full 254-bit scalar, 0 / 1 the GLV half k1 / k2 (|k_h|, sign in *neg).
// Returns the window count; d[w] = the signed digit of window w of |k_h|, read back from the entries msm_recode_store writes.
int hs_msm_digits(const uint8_t* k_be, int c, int half, int32_t* d, int* neg) {
  uint32_t k[8];
  msm_scalar_words(k_be, k);
  const int bits = half < 0 ? 254 : 128, W = msm_windows(bits, c);
  std::vector<uint32_t> key(W), val(W);
  bool ng = false;
  if (half < 0) msm_recode_store<8>(k, c, W, false, true, 0, key.data(), val.data(), 1);
  else {
    const GlvSplit g = glv_split(k);
    ng = half ? g.neg2 : g.neg1;
    msm_recode_store<4>(half ? g.k2 : g.k1, c, W, ng, true, 0, key.data(), val.data(), 1);
  }
  for (int w = 0; w < W; ++w) {
    const int32_t mag = key[w] == MSM_NO_KEY ? 0 : (int32_t)key[w] + 1;
    const bool point_neg = (val[w] & 1u) != 0;          // the sign folded into the point = digit sign XOR the half's sign
    d[w] = (point_neg != ng) ? -mag : mag;
  }
  *neg = ng ? 1 : 0;
  return W;
}

// P + Q with P projective (from the affine encoding, identity allowed) and Q affine (not the identity), by proj_madd
void hs_msm_madd_g1(const uint8_t* p, const uint8_t* q, uint8_t* out) {
  bool o;
  const G1A a = g1_decode(p, o), b = g1_decode(q, o);
  g1_encode(out, g1_to_affine(proj_madd(proj_from_affine(a), b.x, b.y)));
}
void hs_msm_madd_g2(const uint8_t* p, const uint8_t* q, uint8_t* out) {
  bool o;
  const G2A a = g2_decode(p, o), b = g2_decode(q, o);
  g2_encode(out, g2_to_affine(proj_madd(proj_from_affine(a), b.x, b.y)));
}

}  // extern "C"

// the device pipeline on the host: recode (as k_msm_g{1,2}_prep), counting sort (as k_kd_msm_hist / k_scan_excl /
// k_kd_msm_scatter), the bucket levels (msm_bucket_lane), the reduction (msm_reduce_lane), Horner (as k_msm_g{1,2}_final)
template <class F> static void run(const uint8_t* in, const uint8_t* sc, size_t n, int c, uint8_t* out) {
  constexpr bool g2 = FLimbs<F>::n == 2 * NL;
  constexpr int K = FLimbs<F>::n;
  const int halves = g2 ? 1 : 2, bits = g2 ? 254 : 128;
  const uint32_t W = msm_windows(bits, c), B = 1u << (c - 1), u = W * B;
  const size_t S = halves * n, E = S * W;
  std::vector<int32_t> pts(S * 2 * K);
  std::vector<uint32_t> key(E), val(E);
  for (size_t i = 0; i < n; ++i) {
    uint32_t k[8];
    msm_scalar_words(sc + 32 * i, k);
    bool ok;
    if constexpr (!g2) {
      const G1A p = g1_decode(in + 64 * i, ok);
      msm_store(pts.data() + i, S, p.x); msm_store(pts.data() + NL * S + i, S, p.y);
      msm_store(pts.data() + n + i, S, fp_mul(p.x, fp_const(bnc::GLV_BETA))); msm_store(pts.data() + NL * S + n + i, S, p.y);
      const GlvSplit g = glv_split(k);
      msm_recode_store<4>(g.k1, c, W, g.neg1, !p.inf, (uint32_t)i, key.data() + i, val.data() + i, S);
      msm_recode_store<4>(g.k2, c, W, g.neg2, !p.inf, (uint32_t)(n + i), key.data() + n + i, val.data() + n + i, S);
    } else {
      const G2A p = g2_decode(in + 128 * i, ok);
      msm_store(pts.data() + i, S, p.x); msm_store(pts.data() + K * S + i, S, p.y);
      msm_recode_store<8>(k, c, W, false, !p.inf, (uint32_t)i, key.data() + i, val.data() + i, S);
    }
  }
  std::vector<uint32_t> hist(u, 0), end(u), sorted(E);
  for (size_t e = 0; e < E; ++e) if (key[e] != MSM_NO_KEY) ++hist[(e / S) * B + key[e]];
  uint32_t run_ = 0;
  for (uint32_t b = 0; b < u; ++b) { end[b] = run_; run_ += hist[b]; }
  for (size_t e = 0; e < E; ++e) if (key[e] != MSM_NO_KEY) sorted[end[(e / S) * B + key[e]]++] = val[e];
  int levels = 0;
  while (((size_t)1 << (MSM_LG_CHUNK * (levels + 1))) < S) ++levels;
  std::vector<int32_t> part[2], bsum((size_t)u * 3 * K);
  const int32_t* in_ws = nullptr; size_t in_st = 1;
  for (int lv = 0; lv <= levels; ++lv) {
    const bool fin = lv == levels;
    const size_t nslots = fin ? u : (E >> (MSM_LG_CHUNK * (lv + 1))) + u + 1;
    int32_t* out_ws;
    if (fin) out_ws = bsum.data();
    else { part[lv & 1].assign(nslots * 3 * K, 0); out_ws = part[lv & 1].data(); }
    for (size_t s = 0; s < nslots; ++s)
      msm_bucket_lane<F>((uint32_t)s, lv, fin, hist.data(), end.data(), u, sorted.data(), pts.data(), S, in_ws, in_st, out_ws, nslots);
    in_ws = out_ws; in_st = nslots;
  }
  const uint32_t G = B < (uint32_t)MSM_MAX_SEGS ? B : (uint32_t)MSM_MAX_SEGS;
  std::vector<int32_t> seg((size_t)W * G * 3 * K);
  for (uint32_t w = 0; w < W; ++w)
    for (uint32_t g = 0; g < G; ++g) msm_reduce_lane<F>(w, g, B, G, c, bsum.data(), u, seg.data(), (size_t)W * G);
  Proj<F> acc = proj_identity<F>();
  for (uint32_t w = W; w-- > 0;) {
    for (int d = 0; d < c; ++d) acc = proj_dbl(acc);
    for (uint32_t g = 0; g < G; ++g) acc = proj_add(acc, msm_load_p<F>(seg.data() + (size_t)w * G + g, (size_t)W * G));
  }
  if constexpr (g2) g2_encode(out, g2_to_affine(acc));
  else g1_encode(out, g1_to_affine(acc));
}
extern "C" {
void hs_msm_g1(const uint8_t* pts, const uint8_t* sc, size_t n, int c, uint8_t* out) { run<Fp>(pts, sc, n, c, out); }
void hs_msm_g2(const uint8_t* pts, const uint8_t* sc, size_t n, int c, uint8_t* out) { run<Fp2>(pts, sc, n, c, out); }

}  // extern "C"
