// inflate_host.cpp -- inflate.h (fp2_sqrt2, g1_inflate, g2_inflate) compiled for the host with -DBN_CHECK (interval checker and
// operation counters on), as tests/hostsim/unit_pairs_host.cpp does for its headers, beside the codecs they are measured
// against (g1_decompress, g2_decompress).  Used by tests/test_inflate_host.py.  TEST TOOL ONLY.
#include "../../bls-bn254_amd/csrc/inflate.h"
#include <cstring>

using namespace bn;

namespace {
// counts[0..5] = fp_mul, fp_sqr, fp_dot2, fp_norm, fp_lc passes, fp_lc terms (the layout of op_trim_host.cpp)
void snap(double* out) {
  CheckStats& s = check_stats();
  out[0] = (double)s.muls; out[1] = (double)s.sqrs; out[2] = (double)s.dots; out[3] = (double)s.norms; out[4] = (double)s.lcs; out[5] = (double)s.lc_terms;
  check_stats() = CheckStats();
}
}  // namespace

extern "C" {

// a = c0 | c1 (32 big-endian bytes each, canonical).  out = the root found, same layout; returns is_sq.
int hs_inf_fp2_sqrt2(const uint8_t* a, uint8_t* out) {
  bool o0, o1, sq;
  Fp2 x;
  x.c0 = fp_from_be(a, o0); x.c1 = fp_from_be(a + 32, o1);
  if (!o0 || !o1) return -1;
  const Fp2 r = fp2_sqrt2(x, sq);
  fp_to_be(out, r.c0); fp_to_be(out + 32, r.c1);
  return sq ? 1 : 0;
}
int hs_inf_g1(const uint8_t* in, uint8_t* out, double* counts) {
  check_stats() = CheckStats();
  const bool ok = g1_inflate(in, out);
  snap(counts);
  return ok ? 1 : 0;
}
int hs_inf_g2(const uint8_t* in, uint8_t* out, double* counts) {
  check_stats() = CheckStats();
  const bool ok = g2_inflate(in, out);
  snap(counts);
  return ok ? 1 : 0;
}
// the codecs of curve.h on the same input, encoded as k_g1_codec / k_g2_codec encode them, with their counts
int hs_inf_g1_decompress(const uint8_t* in, uint8_t* out, double* counts) {
  bool ok;
  check_stats() = CheckStats();
  const G1A p = g1_decompress(in, ok);
  g1_encode(out, p);
  snap(counts);
  return ok ? 1 : 0;
}
int hs_inf_g2_decompress(const uint8_t* in, uint8_t* out, double* counts) {
  bool ok;
  check_stats() = CheckStats();
  const G2A q = g2_decompress(in, ok);
  g2_encode(out, q);
  snap(counts);
  return ok ? 1 : 0;
}

}  // extern "C"
