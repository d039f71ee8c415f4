// keyset_wire_host.cpp -- the lane functions behind the wire-format forms of the checked aggregation calls, compiled for the host
// with -DBN_CHECK (every field operation asserts the lazy-limb interval discipline, the operation counters are on):
// g1_inflate_point (csrc/inflate.h), ka_scan_wire / ka_wire_out (csrc/keyset_agg.h) and kca_scan_wire
// (csrc/keyset_committee_agg.h), each beside the function it has to agree with.  Used by tests/test_keyset_wire_host.py.
// TEST TOOL ONLY.
#include "../../bls-bn254_amd/csrc/keyset_committee_agg.h"
#include <cstring>

using namespace bn;

namespace {
// counts[0..5] = fp_mul, fp_sqr, fp_dot2, fp_norm, fp_lc passes, fp_lc terms (the layout of inflate_host.cpp)
void snap(double* out) {
  CheckStats& s = check_stats();
  out[0] = (double)s.muls; out[1] = (double)s.sqrs; out[2] = (double)s.dots; out[3] = (double)s.norms; out[4] = (double)s.lcs; out[5] = (double)s.lc_terms;
  check_stats() = CheckStats();
}
// a scan's point in canonical form: the 64 bytes of its affine encoding (the identity as (0, 1))
void canon(uint8_t* out, const G1P& p) { g1_encode(out, g1_to_affine(p)); }
}  // namespace

extern "C" {

// g1_inflate_point: the point encoded as g1_encode writes it (out64), ok returned, the counts of the call alone
int hs_kw_inflate_point(const uint8_t* in, uint8_t* out64, int* inf, double* counts) {
  bool ok;
  check_stats() = CheckStats();
  const G1A p = g1_inflate_point(in, ok);
  snap(counts);
  g1_encode(out64, p);
  *inf = p.inf ? 1 : 0;
  return ok ? 1 : 0;
}
// g1_inflate on the same input: the bytes and ok
int hs_kw_inflate(const uint8_t* in, uint8_t* out64) { return g1_inflate(in, out64) ? 1 : 0; }

// ka_scan_wire on entry s of 32-byte entries / ka_scan on entry s of 64-byte entries: the candidate bit returned, the point in
// canonical form, the counts of the scan alone
int hs_kw_scan_wire(const uint8_t* key_valid, const uint32_t* idx, const uint8_t* wire, const uint8_t* mask, uint32_t s, uint8_t* pt64, double* counts) {
  check_stats() = CheckStats();
  const KaScan r = ka_scan_wire(key_valid, idx, wire, mask, s);
  snap(counts);
  canon(pt64, r.p);
  return r.cand ? 1 : 0;
}
int hs_kw_scan(const uint8_t* key_valid, const uint32_t* idx, const uint8_t* sigs, const uint8_t* mask, uint32_t s, uint8_t* pt64) {
  const KaScan r = ka_scan(key_valid, idx, sigs, mask, s);
  canon(pt64, r.p);
  return r.cand ? 1 : 0;
}
// the committee forms: cvalid = the committee's validity words
int hs_kw_cscan_wire(const uint32_t* cvalid, const uint32_t* pos, const uint8_t* wire, const uint8_t* mask, uint32_t s, uint8_t* pt64, double* counts) {
  check_stats() = CheckStats();
  const KaScan r = kca_scan_wire(cvalid, pos, wire, mask, s);
  snap(counts);
  canon(pt64, r.p);
  return r.cand ? 1 : 0;
}
int hs_kw_cscan(const uint32_t* cvalid, const uint32_t* pos, const uint8_t* sigs, const uint8_t* mask, uint32_t s, uint8_t* pt64) {
  const KaScan r = kca_scan(cvalid, pos, sigs, mask, s);
  canon(pt64, r.p);
  return r.cand ? 1 : 0;
}

// The sum of n entries as the kernels form it -- every entry through ka_scan_wire (all keys valid, no mask), added with
// proj_add, stored and loaded through the workspace layout -- then ka_wire_out: the 64 and the 32 bytes.  n == 0: the identity.
void hs_kw_sum_out(const uint8_t* wire, uint32_t n, uint8_t* full, uint8_t* out32) {
  const uint8_t valid[1] = {1};
  std::vector<uint32_t> idx(n ? n : 1, 0);
  G1P acc = proj_identity<Fp>();
  for (uint32_t s = 0; s < n; ++s) acc = proj_add(acc, ka_scan_wire(valid, idx.data(), wire, nullptr, s).p);
  int32_t ws[3 * NL * 2];
  ka_store_point(ws + 1, 2, acc);                       // stride 2, lane 1
  ka_wire_out(ka_load_point(ws + 1, 2), full, out32);
}

}  // extern "C"
