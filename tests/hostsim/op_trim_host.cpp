// op_trim_host.cpp -- the trimmed operations of the verify hot path compiled for the host with -DBN_CHECK (interval checker and
// operation counters on), as tests/hostsim/hostsim.cpp does for the rest: the prepared Miller loop (unchanged; its counts and
// its bytes after the final exponentiation are pinned), the verdict form of the last final-exponentiation step, the t^x chain
// table, the fixed chain of the hash's square-root power and the constant first SHA-256 state of expand_message_xmd.  Used by tests/test_op_trim.py and scripts/op_trim_counts.py.
// TEST TOOL ONLY.
#define BN_WANT_UNIT_LINE_TABLE
#define BN_LINE_TABLE_QUAL static const
#include "../../bls-bn254_amd/csrc/lane_ops.h"
#include <cstring>

using namespace bn;

namespace {
// counts[0..5] = fp_mul, fp_sqr, fp_dot2, fp_norm, fp_lc passes, fp_lc terms; counts[6] = SHA-256 compressions
void snap(double* out) {
  CheckStats& s = check_stats();
  out[0] = (double)s.muls; out[1] = (double)s.sqrs; out[2] = (double)s.dots; out[3] = (double)s.norms; out[4] = (double)s.lcs; out[5] = (double)s.lc_terms;
  out[6] = (double)s.sha_blocks;
  check_stats() = CheckStats();
}
// the key's 88 unit entries the way k_g2_prepare + k_g2_expand leave them (b3^-1 four entries at a time)
int unit_table(const G2A& Q, int32_t* raw, int32_t* tab) {
  g2_prepare_lines(Q, Ws{raw, 1, 0, false});
  int zeros = 0;
  for (int t = 0; t < 88; t += 4) {
    Fp2 x[4];
    bool zero[4];
    for (int q = 0; q < 4; ++q) x[q] = fp2_load_limbs(Ws{raw + 54 * (t + q) + 18, 1, 0, false});
    fp2_inv4(x, zero);
    for (int q = 0; q < 4; ++q) {
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
// the five phase values of the hard part for f, in the phase buffers' form (canonical limbs read back as fp12_load_mem does)
void phase_values(const Fp12& f, int32_t* ws, Ws* w, Fp12* vals) {
  Fp12 &t = vals[0], &a = vals[1], &c = vals[2], &b2 = vals[3], &x0 = vals[4], b, d2;
  t = fe_easy(f);
  fe_h1(cyclotomic_exp_x(t), a, b);
  fe_h2(cyclotomic_exp_x(b), b, c, b2, d2);
  x0 = cyclotomic_exp_x(d2);
  for (int k = 0; k < 5; ++k) {
    w[k] = Ws{ws + 108 * k, 1, 0, false};
    fp12_store_limbs(ws + 108 * k, 1, vals[k]);
    fp12_store_mem(w[k], fp12_load_limbs(ws + 108 * k, 1));
  }
}
}  // namespace

extern "C" {

// final_exponentiation(miller_loop_prepared_unit(...)) for (sig, H, pk) as k_g2_prepare + k_g2_expand + k_miller_prepared run it, H =
// (x z : y z : z) with z = the Montgomery form of z_small.  counts: the loop alone.  Returns the number of zero b3 (0 for a
// key of the r-torsion), -1 when an input does not decode, -2 when the tuple's inversion did not finish.
int hs_ot_miller(const uint8_t* sig, const uint8_t* h, const uint8_t* pk, int z_small, uint8_t* gt_out, double* counts) {
  bool o1, o2, o3;
  G1A S = g1_decode(sig, o1), H = g1_decode(h, o2);
  G2A Q = g2_decode(pk, o3);
  if (!o1 || !o2 || !o3) return -1;
  static int32_t raw[88 * 54], tab[88 * 162], cwm[72];
  const int zeros = unit_table(Q, raw, tab);
  Fp z = fp_one();
  for (int k = 1; k < z_small; ++k) z = fp_norm(fp_add(z, fp_one()));
  z = fp_canon(z);
  const Fp xs = fp_norm(S.x), ys = fp_norm(S.y), X = fp_mul(fp_norm(H.x), z), Y = fp_mul(fp_norm(H.y), z), Z = z;
  const Ws cw = {cwm, 1, 0, false};
  bool inv_ok;
  const bool unit = miller_unit_coords(xs, ys, X, Y, Z, cw, inv_ok);
  if (!inv_ok) return -2;
  check_stats() = CheckStats();
  const Fp12 f = miller_loop_prepared_unit(cw, Ws{tab, 1, 0, false}, unit);
  snap(counts);
  fp12_to_be(gt_out, final_exponentiation(f));
  return zeros;
}
// The last step of the final exponentiation on the Miller value `in`, both ways.  full: the eight-step interpreter (the Gt
// modes of k_fe_h3) and fp12_is_one, cross-checked with the register form fe_h3.  verdict: seven steps and fe_h3_verdict (the
// verify modes).  coeff in 0..11 adds one to that Fp coefficient of the parked eighth factor l3^(p^3) before both decide, so
// that the two sides differ in exactly one coefficient; then full = fp12_is_one(A * B').  Returns 0, or -1 when the register
// form and the interpreter disagree.  dense_counts: one fp12_mul_mem on its own.
int hs_ot_h3(const uint8_t* in, int coeff, int* verdict, int* full, double* verdict_counts, double* full_counts, double* dense_counts) {
  bool ok;
  static int32_t ws[108 * 5], tmp[108 * 4], park[108];
  Ws w[5];
  Fp12 vals[5];
  phase_values(fp12_from_be(in, ok), ws, w, vals);
  const Ws pk = {park, 1, 0, false}, tw = {tmp, 1, 0, false};
  check_stats() = CheckStats();
  Fp12 r8 = fe_h3_loop(w, tw, &pk, 8);
  bool one8 = fp12_is_one(r8);
  snap(full_counts);
  uint8_t b1[384], b2[384];
  fp12_to_be(b1, fe_h3(vals[0], vals[1], vals[2], vals[3], vals[4])); fp12_to_be(b2, r8);
  if (std::memcmp(b1, b2, 384) != 0) return -1;
  check_stats() = CheckStats();
  Fp12 r7 = fe_h3_loop(w, tw, &pk, 7);
  *verdict = fe_h3_verdict(r7, tw) ? 1 : 0;
  snap(verdict_counts);
  if (coeff >= 0) {
    const Ws c = ws_at(tw, 324 + 9 * (size_t)coeff);
    fp_store_mem(c, fp_norm(fp_add(fp_load_mem(c), fp_one())));
    *verdict = fe_h3_verdict(r7, tw) ? 1 : 0;
    one8 = fp12_is_one(fp12_mul_mem(r7, ws_at(tw, 324), &pk));
  }
  *full = one8 ? 1 : 0;
  check_stats() = CheckStats();
  (void)fp12_mul_mem(r7, ws_at(tw, 324), &pk);
  snap(dense_counts);
  return 0;
}
// fe_h3_verdict on the all-zero phase values (f = 0): the two sides agree there and the verdict must still be "not one"
int hs_ot_h3_zero() {
  static int32_t ws[108 * 5], tmp[108 * 4], park[108];
  Ws w[5];
  const Fp12 z = {{fp2_zero(), fp2_zero(), fp2_zero()}, {fp2_zero(), fp2_zero(), fp2_zero()}};
  for (int k = 0; k < 5; ++k) { w[k] = Ws{ws + 108 * k, 1, 0, false}; fp12_store_mem(w[k], z); }
  const Ws pk = {park, 1, 0, false}, tw = {tmp, 1, 0, false};
  const Fp12 r7 = fe_h3_loop(w, tw, &pk, 7);
  return (fe_h3_verdict(r7, tw) ? 1 : 0) | (fp12_is_one(fe_h3_loop(w, tw, &pk, 8)) ? 2 : 0);
}

// the t^x chain table itself (5 signed bytes per op: load, sq, mul, store, cstore), for a check with Python integers
int hs_ot_chain_table(int8_t* out, int* slots) {
  const ChainOp prog[BN_X_CHAIN_LEN] = BN_X_CHAIN;
  for (int k = 0; k < BN_X_CHAIN_LEN; ++k) {
    out[5 * k] = prog[k].load; out[5 * k + 1] = prog[k].sq; out[5 * k + 2] = prog[k].mul; out[5 * k + 3] = prog[k].store; out[5 * k + 4] = prog[k].cstore;
  }
  *slots = BN_X_CHAIN_SLOTS;
  return BN_X_CHAIN_LEN;
}
// one t^x chain as k_fe_expx runs it, on the easy part of `in`; 1 when it equals the binary ladder
int hs_ot_expx(const uint8_t* in, double* counts) {
  bool ok;
  Fp12 t = fe_easy(fp12_from_be(in, ok));
  static int32_t slots[108 * 10], park[108];
  const Ws pk = {park, 1, 0, false};
  check_stats() = CheckStats();
  Fp12 c = cyclotomic_exp_x_chain(t, Ws{slots, 1, 0, false}, &pk);
  snap(counts);
  uint8_t ba[384], bc[384];
  fp12_to_be(ba, cyclotomic_exp_x(t)); fp12_to_be(bc, c);
  return std::memcmp(ba, bc, 384) == 0;
}

// a^((p-3)/4) by the fixed chain (out) and by fp_pow's 4-bit windows (out_win), with the counts of each
void hs_ot_pow_pm3_4(const uint8_t* a, uint8_t* out, uint8_t* out_win, double* counts, double* win_counts) {
  bool o;
  const Fp x = fp_from_be(a, o);
  check_stats() = CheckStats();
  const Fp r = fp_pow_pm3_4(x);
  snap(counts);
  const Fp v = fp_pow(x, BN_EXP(EXP_PM3_4));
  snap(win_counts);
  fp_to_be(out, r); fp_to_be(out_win, v);
}

// the state that expand_message_xmd starts b_0 from
void hs_ot_sha_zpad_state(uint32_t* out) {
  Sha256 s;
  sha256_init_zpad(s);
  for (int i = 0; i < 8; ++i) out[i] = s.h[i];
}
// one hash as the verify pipeline runs it (k_hash_to_g1 mode 3: homogeneous output), with its counts; out = the affine point
void hs_ot_hash(const uint8_t* msg, size_t len, const uint8_t* dst, uint32_t dst_len, uint8_t* out, double* counts) {
  check_stats() = CheckStats();
  const G1P hp = lane_hash_to_g1_proj(msg, len, dst, dst_len);
  snap(counts);
  g1_encode(out, g1_to_affine(hp));
}

}  // extern "C"
