// unit_pairs_host.cpp -- the unit-coefficient line pairs of the prepared-key verify path (pairing.h: fp2_inv4,
// line_pair_expand_unit, miller_unit_coords, miller_loop_prepared_unit) compiled for the host with -DBN_CHECK, as
// tests/hostsim/hostsim.cpp does for the rest.  Used by tests/test_unit_pairs.py.  TEST TOOL ONLY.
#define BN_WANT_UNIT_LINE_TABLE
#define BN_LINE_TABLE_QUAL static const
#include "../../bls-bn254_amd/csrc/lane_ops.h"
#include "../../bls-bn254_amd/csrc/tri.h"
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include "../../bls-bn254_amd/csrc/wide.h"
#include <vector>
#include <cstring>

using namespace bn;

// tri.h on the host, as in hostsim.cpp: the four lanes of a quad run as four threads; a DPP fetch is a rendezvous
namespace {
struct TriQuad {
  bn::Fp slot[4];
  std::mutex m; std::condition_variable cv; int arrived = 0; long gen = 0;
  void barrier() {
    std::unique_lock<std::mutex> lk(m);
    const long g = gen;
    if (++arrived == 4) { arrived = 0; ++gen; cv.notify_all(); }
    else cv.wait(lk, [&] { return gen != g; });
  }
};
thread_local TriQuad* tri_quad = nullptr;
thread_local uint32_t tri_quad_role = 0;
void tri_run(const std::function<void(uint32_t)>& fn) {
  TriQuad q;
  std::thread th[4];
  for (uint32_t r = 0; r < 4; ++r) th[r] = std::thread([&, r] { tri_quad = &q; tri_quad_role = r; fn(r); });
  for (auto& t : th) t.join();
}
}  // namespace
namespace bn {
void tri_host_run4(void (*fn)(void*, uint32_t), void* arg) { tri_run([&](uint32_t role) { fn(arg, role); }); }
uint32_t tri_host_role() { return tri_quad_role; }
Fp tri_host_fetch(const Fp& x, int p0, int p1, int p2, int p3) {
  const int perm[4] = {p0, p1, p2, p3};
  tri_quad->slot[tri_quad_role] = x;
  tri_quad->barrier();
  Fp r = tri_quad->slot[perm[tri_quad_role]];
  tri_quad->barrier();
  return r;
}
}  // namespace bn

namespace {
// the key's 88 unit entries the way k_g2_prepare + k_g2_expand leave them: b3^-1 four entries at a time; returns the zero b3 count
int unit_table(const G2A& Q, int32_t* raw, int32_t* tab) {
  g2_prepare_lines(Q, Ws{raw, 1, 0, false});
  int zeros = 0;
  for (int t = 0; t < 88; t += 4) {
    Fp2 x[4];
    bool zero[4];
    for (int q = 0; q < 4; ++q) x[q] = fp2_load_limbs(Ws{raw + 54 * (t + q) + 18, 1, 0, false});
    fp2_inv4(x, zero);
    for (int q = 0; q < 4; ++q) {
      // through memory as the kernel passes it on: the multiplier's limbs stored as they are, read back as a lazy entry
      int32_t park[18];
      for (int l = 0; l < NL; ++l) { park[l] = x[q].c0.l[l]; park[NL + l] = x[q].c1.l[l]; }
      zeros += zero[q] ? 1 : 0;
      const Ws bw = {raw + 54 * (t + q), 1, 0, false};
      line_pair_expand_unit(BN_NEG_G2_UNIT_LINE_TABLE[t + q], fp2_load_limbs(bw), fp2_load_limbs_lazy(Ws{park, 1, 0, false}), fp2_load_limbs(ws_at(bw, 36)),
                            Ws{tab + 162 * (t + q), 1, 0, false});
    }
  }
  return zeros;
}
void snap(double* out) {
  CheckStats& s = check_stats();
  out[0] = (double)s.muls; out[1] = (double)s.sqrs; out[2] = (double)s.dots; out[3] = (double)s.norms; out[4] = (double)s.lcs; out[5] = (double)s.lc_terms;
  check_stats() = CheckStats();
}
}  // namespace

extern "C" {

// The digit of the loop's NAF(6x+2) at position j, as the device reads it (ate_naf_digit), and the table's length
int hs_ate_naf_len() { return bnc::ATE_NAF_LEN; }
int hs_ate_naf_digit(int j) { return ate_naf_digit(j); }

// final_exponentiation(miller_loop_prepared_unit(...)) for (sig, H, pk) the way k_g2_prepare + k_g2_expand + k_miller_prepared run it:
// the key's raw lines, b3^-1 four entries at a time (fp2_inv4), the unit entries, the scaled coordinate values, the loop.
// H = (x z : y z : z) with z = the Montgomery form of z_small; h_identity: H = (0 : y : 0) instead (the lane with X = 0).
// pk is taken as it decodes (a point outside the subgroup runs the same formulas).  Returns the number of entries whose b3 was
// zero (the kernel clears key_ok for them), -1 when an input does not decode, -2 when the tuple's inversion did not finish.
// counts[0..5]: executed fp_mul, fp_sqr, fp_dot2, fp_norm, fp_lc passes, fp_lc terms of the loop; counts[6..11]: of the prologue
// (miller_unit_coords; its divstep inversion is not made of these operations and is not in the counts).
int hs_unit_verify(const uint8_t* sig, const uint8_t* h, const uint8_t* pk, int z_small, int h_identity, uint8_t* gt_out, double* counts) {
  bool o1, o2, o3;
  G1A S = g1_decode(sig, o1), H = g1_decode(h, o2);
  G2A Q = g2_decode(pk, o3);
  if (!o1 || !o2 || !o3) return -1;
  static int32_t raw[88 * 54], tab[88 * 162], cwm[72];
  const int zeros = unit_table(Q, raw, tab);
  Fp z = fp_one();
  for (int k = 1; k < z_small; ++k) z = fp_norm(fp_add(z, fp_one()));
  z = fp_canon(z);
  const Fp xs = fp_norm(S.x), ys = fp_norm(S.y);
  Fp X = fp_mul(fp_norm(H.x), z), Y = fp_mul(fp_norm(H.y), z), Z = z;
  if (h_identity) { X = fp_norm(fp_zero()); Z = fp_norm(fp_zero()); }
  const Ws cw = {cwm, 1, 0, false};
  check_stats() = CheckStats();
  bool inv_ok;
  const bool unit = miller_unit_coords(xs, ys, X, Y, Z, cw, inv_ok);
  if (!inv_ok) return -2;
  snap(counts + 6);
  const Fp12 f = miller_loop_prepared_unit(cw, Ws{tab, 1, 0, false}, unit);
  snap(counts);
  fp12_to_be(gt_out, final_exponentiation(f));
  return zeros;
}
// The other readers of the pair table, unchanged: the quad loop (tri.h, k_miller_tri_prepared) and the wave-per-tuple loop (wide.h,
// k_miller_wide_prepared) evaluate the unit entries at the nine UNSCALED coordinate values (slot 2 times xs X), so their Miller
// values differ from the textbook product by an Fp2 factor per step only.  gt_tri / gt_wide: after the final exponentiation.
int hs_unit_tri_wide(const uint8_t* sig, const uint8_t* h, const uint8_t* pk, int z_small, uint8_t* gt_tri, uint8_t* gt_wide) {
  bool o1, o2, o3;
  G1A S = g1_decode(sig, o1), H = g1_decode(h, o2);
  G2A Q = g2_decode(pk, o3);
  if (!o1 || !o2 || !o3) return -1;
  static int32_t raw[88 * 54], tab[88 * 162], inv[81];
  const int zeros = unit_table(Q, raw, tab);
  Fp z = fp_one();
  for (int k = 1; k < z_small; ++k) z = fp_norm(fp_add(z, fp_one()));
  z = fp_canon(z);
  const Fp xs = fp_norm(S.x), ys = fp_norm(S.y), X = fp_mul(fp_norm(H.x), z), Y = fp_mul(fp_norm(H.y), z), Z = z;
  auto put = [&](const Ws& w) {
    fp_store_mem(w, X); fp_store_mem(ws_at(w, 9), Y); fp_store_mem(ws_at(w, 18), Z);
    fp_store_mem(ws_at(w, 27), fp_mul(xs, X)); fp_store_mem(ws_at(w, 36), fp_mul(ys, Y)); fp_store_mem(ws_at(w, 45), fp_mul(xs, Z));
    fp_store_mem(ws_at(w, 54), fp_mul(ys, Z)); fp_store_mem(ws_at(w, 63), fp_mul(ys, X)); fp_store_mem(ws_at(w, 72), fp_mul(xs, Y));
  };
  const Ws w = {inv, 1, 0, false}, tw = {tab, 1, 0, false};
  put(w);
  Fp6 res[4];
  tri_run([&](uint32_t role) { res[role] = tri_miller_prepared(w, tw, role); });
  fp12_to_be(gt_tri, final_exponentiation(Fp12{res[0], res[1]}));
  std::vector<int32_t> lds(WIDE_LDS_DWORDS, 0), col(256, 0);
  Wide W{lds.data()};
  const Ws cw = {col.data() + 32, 1, 0, false};
  put(cw);
  wide_miller_prepared(W, tw, cw, true);
  const Fp12 fw = {{fp2_load_mem(wide_val(W, WV_R, 0)), fp2_load_mem(wide_val(W, WV_R, 1)), fp2_load_mem(wide_val(W, WV_R, 2))},
                   {fp2_load_mem(wide_val(W, WV_R, 3)), fp2_load_mem(wide_val(W, WV_R, 4)), fp2_load_mem(wide_val(W, WV_R, 5))}};
  fp12_to_be(gt_wide, final_exponentiation(fw));
  return zeros;
}
// slot 2 of every unit entry holds the Montgomery form of one (canonical limbs): 1 when it does for all 88 entries of the key
int hs_unit_slot2_is_one(const uint8_t* pk) {
  bool ok;
  G2A Q = g2_decode(pk, ok);
  if (!ok) return -1;
  static int32_t raw[88 * 54], ent[162];
  g2_prepare_lines(Q, Ws{raw, 1, 0, false});
  for (int t = 0; t < 88; ++t) {
    const Ws bw = {raw + 54 * t, 1, 0, false};
    line_pair_expand_unit(BN_NEG_G2_UNIT_LINE_TABLE[t], fp2_load_limbs(bw), fp2_inv(fp2_load_limbs(ws_at(bw, 18))), fp2_load_limbs(ws_at(bw, 36)), Ws{ent, 1, 0, false});
    for (int l = 0; l < NL; ++l) if (ent[36 + l] != bnc::ONE[l] || ent[45 + l] != 0) return 0;
  }
  return 1;
}
// fp2_inv4 against fp2_inv: four values (64 bytes each: c0, c1 big endian); 1 when every x_i^-1 agrees and zero[] marks exactly the zeros
int hs_fp2_inv4_matches(const uint8_t* in) {
  Fp2 x[4], y[4];
  bool zero[4], ok = true;
  for (int i = 0; i < 4; ++i) { x[i] = fp2_from_be(in + 64 * i, ok); y[i] = x[i]; }
  if (!ok) return -1;
  fp2_inv4(x, zero);
  for (int i = 0; i < 4; ++i) {
    if (zero[i] != fp2_is_zero(y[i])) return 0;
    if (!fp2_eq(x[i], fp2_inv(y[i]))) return 0;
  }
  return 1;
}

}  // extern "C"
