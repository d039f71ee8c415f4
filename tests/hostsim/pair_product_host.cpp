// pair_product_host.cpp -- one step of the prepared Miller loop (pairing.h: ell_pair_unit, the twelve-product form of f times a
// unit line pair) compiled for the host with -DBN_CHECK, on operands given limb by limb together with the interval the checker is
// to carry for them.  Used by tests/test_pair_product.py.  TEST TOOL ONLY.
#include "../../bls-bn254_amd/csrc/pairing.h"
#include <cstring>

using namespace bn;

namespace {
void snap(double* out) {
  CheckStats& s = check_stats();
  out[0] = (double)s.muls; out[1] = (double)s.sqrs; out[2] = (double)s.dots; out[3] = (double)s.norms; out[4] = (double)s.lcs; out[5] = (double)s.lc_terms;
  check_stats() = CheckStats();
}
Fp fp_raw(const int32_t* l, const double* t, const char* what) {      // t: lo, hi, tlo, thi, vb
  Fp r;
  for (int i = 0; i < NL; ++i) r.l[i] = l[i];
  set_trk(r, t[0], t[1], t[2], t[3], t[4]);
  check_actual(r, what);
  return r;
}
Fp12 fp12_raw(const int32_t* l, const double* t) {                   // 12 x 9 limbs: c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1
  Fp c[12];
  for (int k = 0; k < 12; ++k) c[k] = fp_raw(l + NL * k, t, "f operand");
  return {{{c[0], c[1]}, {c[2], c[3]}, {c[4], c[5]}}, {{c[6], c[7]}, {c[8], c[9]}, {c[10], c[11]}}};
}
void widen(double* w, const Fp& a, bool first) {
  if (first) { w[0] = a.lo; w[1] = a.hi; w[2] = a.tlo; w[3] = a.thi; w[4] = a.vb; return; }
  w[0] = std::fmin(w[0], a.lo); w[1] = std::fmax(w[1], a.hi); w[2] = std::fmin(w[2], a.tlo); w[3] = std::fmax(w[3], a.thi); w[4] = std::fmax(w[4], a.vb);
}
void widen12(double* w, const Fp12& f, bool first) {
  const Fp2* c[6] = {&f.c0.c0, &f.c0.c1, &f.c0.c2, &f.c1.c0, &f.c1.c1, &f.c1.c2};
  for (int k = 0; k < 6; ++k) { widen(w, c[k]->c0, first && k == 0); widen(w, c[k]->c1, false); }
}
void put_cw(const int32_t* cw, const double* t, int32_t* mem) {
  for (int k = 0; k < 8; ++k) fp_store_mem(Ws{mem + NL * k, 1, 0, false}, fp_raw(cw + NL * k, t, "coordinate value"));
}
}  // namespace

extern "C" {

// The intervals the checker carries where the loop runs (lo, hi, tlo, thi, vb each; data independent):
//   out[0..4]   a coefficient of f as fp12_sqr leaves it (widest of the twelve), f being the value of a pair step
//   out[5..9]   a coefficient of f as ell_pair_unit leaves it (two steps follow each other at a non-zero digit and at the end)
//   out[10..14] a coordinate value as miller_unit_coords parks it (widest of the eight)
// entry: 162 limbs, xy: five canonical Montgomery values xs, ys, X, Y, Z (any non-zero field elements; only their intervals matter)
int hs_pp_bounds(const int32_t* entry, const int32_t* xy, double* out) {
  static int32_t cwm[72], ent[162];
  std::memcpy(ent, entry, sizeof ent);
  Fp v[5];
  for (int k = 0; k < 5; ++k) v[k] = fp_norm(fp_from_limbs(xy + NL * k));
  const Ws cw = {cwm, 1, 0, false};
  bool ok;
  const bool unit = miller_unit_coords(v[0], v[1], v[2], v[3], v[4], cw, ok);
  if (!ok) return -2;
  for (int k = 0; k < 8; ++k) widen(out + 10, fp_load_mem(ws_at(cw, NL * k)), k == 0);
  Fp12 f = fp12_one();
  const Ws e = {ent, 1, 0, false};
  for (int it = 0; it < 4; ++it) {                       // the intervals repeat from the second round on
    f = fp12_sqr(f);
    widen12(out, f, it == 0);
    f = ell_pair_unit(f, e, cw, unit);
    widen12(out + 5, f, it == 0);
    f = ell_pair_unit(f, e, cw, unit);
    widen12(out + 5, f, false);
  }
  return 0;
}

// One pair step.  f: 108 limbs (tower order), ftrk: its interval; entry: 162 limbs (read as a table entry, in its declared range);
// cwl: 72 limbs (Y, Z, ys Y, xs Z, ys Z, ys X, xs Y, X), cwtrk: their interval.  out: the twelve coefficients of ell_pair_unit's value,
// canonical, 32 bytes big endian each, tower order.  counts: fp_mul, fp_sqr, fp_dot2, fp_norm, fp_lc passes, fp_lc terms of the step.
int hs_pp_step(const int32_t* fl, const double* ftrk, const int32_t* entry, const int32_t* cwl, const double* cwtrk, int unit, uint8_t* out, double* counts) {
  static int32_t cwm[72], ent[162];
  std::memcpy(ent, entry, sizeof ent);
  put_cw(cwl, cwtrk, cwm);
  const Fp12 f = fp12_raw(fl, ftrk);
  check_stats() = CheckStats();
  const Fp12 r = ell_pair_unit(f, Ws{ent, 1, 0, false}, Ws{cwm, 1, 0, false}, unit != 0);
  snap(counts);
  const Fp2* c[6] = {&r.c0.c0, &r.c0.c1, &r.c0.c2, &r.c1.c0, &r.c1.c1, &r.c1.c2};
  for (int k = 0; k < 6; ++k) { fp_to_be(out + 64 * k, c[k]->c0); fp_to_be(out + 64 * k + 32, c[k]->c1); }
  return 0;
}

// The whole loop on a table of 88 entries (88 x 162 limbs) and 72 limbs of coordinate values: its operation counts (data independent)
int hs_pp_loop_counts(const int32_t* table, const int32_t* cwl, const double* cwtrk, int unit, double* counts) {
  static int32_t cwm[72], tab[88 * 162];
  std::memcpy(tab, table, sizeof tab);
  put_cw(cwl, cwtrk, cwm);
  check_stats() = CheckStats();
  const Fp12 f = miller_loop_prepared_unit(Ws{cwm, 1, 0, false}, Ws{tab, 1, 0, false}, unit != 0);
  snap(counts);
  return f.c0.c0.c0.l[0] == 0x7fffffff ? 1 : 0;          // keeps the loop's value alive
}

}  // extern "C"
