// threshold_batch_host.cpp -- the lane functions of csrc/threshold_batch.h (threshold combine over many groups) compiled for the
// host with -DBN_CHECK (every field operation asserts the lazy-limb interval discipline), for tests/test_threshold_batch_host.py:
// the segmented Lagrange coefficients, the GLV scalar multiplication, and the whole decode -> Lagrange -> multiply -> segmented
// sum -> status pipeline run lane by lane as the kernels of k_threshold_batch.hip index it.  TEST TOOL ONLY.
#include "../../bls-bn254_amd/csrc/threshold_batch.h"
#include <vector>

using namespace bn;

namespace {
constexpr size_t SUM_GROUP = 16;      // points per lane and level of the segmented sum (host_threshold_batch.hip: TH_SUM_GROUP)

// k_fr_decode + k_lagrange_seg over N = off[ng] shares (off[0] = 0), t_big = no hand-over; marks[g] bit 0 as gstat
void lagrange_all(const uint8_t* ids, const uint32_t* off, uint32_t ng, uint8_t* scalars, std::vector<uint32_t>& glv, std::vector<uint32_t>& marks) {
  const size_t N = off[ng];
  std::vector<int32_t> x(9 * N);
  std::vector<uint8_t> ok(N);
  for (size_t i = 0; i < N; ++i) {
    bool o;
    const Fr v = fr_from_be(ids + 32 * i, o);
    th_store_fr(x.data() + i, N, v);
    ok[i] = (o && !fr_is_zero(v)) ? 1 : 0;
  }
  glv.assign(9 * N, 0); marks.assign(ng, 0);
  for (size_t i = 0; i < N; ++i) {
    const uint32_t g = th_find_group(off, ng, (uint32_t)i);
    bool bad;
    const Fr lam = lagrange_seg_lane(x.data(), ok.data(), N, (uint32_t)i, off[g], off[g + 1], bad);
    if (bad) marks[g] |= 1u;
    uint32_t w[8];
    th_fr_words(lam, w);
    if (scalars) for (int j = 0; j < 8; ++j) store_be32(scalars + 32 * i + 4 * (7 - j), w[j]);
    const GlvSplit s = glv_split(w);
    for (int j = 0; j < 4; ++j) { glv[j * N + i] = s.k1[j]; glv[(4 + j) * N + i] = s.k2[j]; }
    glv[8 * N + i] = (s.neg1 ? 1u : 0u) | (s.neg2 ? 2u : 0u);
  }
}
}  // namespace

extern "C" {

// coefficients (32 B big-endian per share) and bad[g] = a bad or repeated id inside group g
void hs_thb_lagrange(const uint8_t* ids, const uint32_t* off, uint32_t ng, uint8_t* scalars, uint8_t* bad) {
  std::vector<uint32_t> glv, marks;
  lagrange_all(ids, off, ng, scalars, glv, marks);
  for (uint32_t g = 0; g < ng; ++g) bad[g] = (uint8_t)(marks[g] & 1u);
}

// out = [k] P by glv_split + g1_smul_glv_lane; returns bit 0: the point was accepted, bits 1, 2: the signs of the halves,
// bits 3, 4: the halves are even
int hs_thb_smul(const uint8_t* point, const uint8_t* k_be, uint8_t* out) {
  uint32_t w[8];
  for (int j = 0; j < 8; ++j) w[j] = load_be32(k_be + 4 * (7 - j));
  const GlvSplit s = glv_split(w);
  bool ok;
  const G1A p = th_point(point, ok);
  std::vector<int32_t> tab(TH_SMUL_TAB_LIMBS);
  const G1P r = g1_smul_glv_lane(p, s, Ws{tab.data(), 1, 0, false});
  g1_encode(out, g1_to_affine(r));
  return (ok ? 1 : 0) | (s.neg1 ? 2 : 0) | (s.neg2 ? 4 : 0) | ((s.k1[0] & 1u) ? 0 : 8) | ((s.k2[0] & 1u) ? 0 : 16);
}

// the same for explicit halves (16 B big-endian magnitudes, neg bit 0 / 1: k1 / k2 negative): out = [+-k1] P + [+-k2] phi(P).
// glv_split of a canonical scalar happens never to give a negative k1; the multiplication must not rely on that.
void hs_thb_smul_halves(const uint8_t* point, const uint8_t* k1_be, const uint8_t* k2_be, int neg, uint8_t* out) {
  GlvSplit s;
  for (int j = 0; j < 4; ++j) { s.k1[j] = load_be32(k1_be + 4 * (3 - j)); s.k2[j] = load_be32(k2_be + 4 * (3 - j)); }
  s.neg1 = (neg & 1) != 0; s.neg2 = (neg & 2) != 0;
  bool ok;
  const G1A p = th_point(point, ok);
  std::vector<int32_t> tab(TH_SMUL_TAB_LIMBS);
  g1_encode(out, g1_to_affine(g1_smul_glv_lane(p, s, Ws{tab.data(), 1, 0, false})));
}

// the whole batch: out[64 g ..] and status[g] as blsbn254_threshold_combine_batch defines them
void hs_thb_combine(const uint8_t* ids, const uint8_t* sigs, const uint32_t* off, uint32_t ng, uint8_t* out, uint8_t* status) {
  const size_t N = off[ng];
  std::vector<uint32_t> glv, marks;
  lagrange_all(ids, off, ng, nullptr, glv, marks);
  std::vector<int32_t> pts(27 * (N ? N : 1)), tab(TH_SMUL_TAB_LIMBS);
  for (size_t i = 0; i < N; ++i) {
    bool ok;
    const G1A p = th_point(sigs + 64 * i, ok);
    if (!ok) marks[th_find_group(off, ng, (uint32_t)i)] |= 2u;
    GlvSplit s;
    for (int j = 0; j < 4; ++j) { s.k1[j] = glv[j * N + i]; s.k2[j] = glv[(4 + j) * N + i]; }
    s.neg1 = (glv[8 * N + i] & 1u) != 0; s.neg2 = (glv[8 * N + i] & 2u) != 0;
    const G1P r = g1_smul_glv_lane(p, s, Ws{tab.data(), 1, 0, false});
    store_fp(pts.data() + i, N, r.x); store_fp(pts.data() + 9 * N + i, N, r.y); store_fp(pts.data() + 18 * N + i, N, r.z);
  }
  for (uint32_t g = 0; g < ng; ++g) {
    // levels of chunk sums as k_g1_seg_sum runs them: canonical limbs between the levels
    std::vector<G1P> cur;
    for (uint32_t i = off[g]; i < off[g + 1]; ++i) cur.push_back({load_fp(pts.data() + i, N), load_fp(pts.data() + 9 * N + i, N), load_fp(pts.data() + 18 * N + i, N)});
    do {
      std::vector<G1P> nxt;
      for (size_t s0 = 0; s0 < cur.size() || nxt.empty(); s0 += SUM_GROUP) {
        G1P acc = proj_identity<Fp>();
        for (size_t j = s0; j < cur.size() && j < s0 + SUM_GROUP; ++j) acc = proj_add(acc, cur[j]);
        int32_t col[27];
        store_fp(col, 1, acc.x); store_fp(col + 9, 1, acc.y); store_fp(col + 18, 1, acc.z);
        nxt.push_back({load_fp(col, 1), load_fp(col + 9, 1), load_fp(col + 18, 1)});
      }
      cur.swap(nxt);
    } while (cur.size() > 1);
    g1_encode(out + 64 * g, g1_to_affine(cur[0]));
    status[g] = (marks[g] & 1u) ? 1 : (marks[g] & 2u) ? 2 : 0;
    if (status[g]) for (int b = 0; b < 64; ++b) out[64 * g + b] = b == 63 ? 1 : 0;
  }
}

}  // extern "C"
