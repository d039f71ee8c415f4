// pairing_check_rlc_host.cpp -- the lane functions of csrc/pairing_check_rlc.h (pairing-product checks over ragged groups by random
// linear combination) and the plain C++ of csrc/pairing_check_rlc_plan.h / aggregate_rlc_plan.h compiled for the host with
// -DBN_CHECK, for tests/test_pairing_check_rlc_host.py.  A STAND-ALONE program: it reads commands from the file named on its
// command line and prints one line of results per command, so a host sanitizer build of it (-fsanitize=address,undefined) runs as
// it is.  TEST TOOL ONLY.
//   digest   dg(hex, 32 bytes)                          -> a b of agr_weight_of_digest
//   weight   seed(hex) g                                -> a b of pcr_weight
//   mul      a b p(hex, 64 bytes)                       -> the encoding of [a + b lambda] P by pcr_mul_glv32, through the stored layouts
//   mul2     a b p(hex) c d q(hex)                      -> the two encodings by pcr_mul_glv32_x2, through the stored layouts
//   pair     g1(hex, 64) g2(hex, 128)                   -> ok skip of pcr_pair, key_ok by the key preparation's test of Q
//   lane     g1(hex) g2(hex) a b elig                   -> what k_pcr_weigh stores for the pair: pcr_pair, the affine layout, the chain, the selection
//   eligible n flag x n                                 -> pcr_eligible
//   round1   N u max_keys                               -> pcr_round1
//   consts                                              -> PCR_SMAX PCR_MERGE_GAP AGR_MAX_SEGMENTS
//   segments setting s_max N u G                        -> agr_segments
//   cut      G S                                        -> the S + 1 bounds, then the G segments
//   ranges   S bound x (S + 1) pass x S G elig x G off x (G + 1) merge_gap -> eligible n_ranges, then first second per range
// Blobs are hex strings; numbers are decimal.
#include "../../bls-bn254_amd/csrc/pairing_check_rlc.h"
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>

using namespace bn;

static std::vector<uint8_t> blob(std::istream& in) {
  std::string s;
  in >> s;
  std::vector<uint8_t> v;
  for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  return v;
}
template <typename T>
static std::vector<T> nums(std::istream& in, size_t n) {
  std::vector<T> v(n);
  for (size_t i = 0; i < n; ++i) { uint64_t x; in >> x; v[i] = (T)x; }
  return v;
}
static void print_hex(const uint8_t* b, size_t n) { for (size_t i = 0; i < n; ++i) std::printf("%02x", b[i]); }
// a point as k_pcr_pairs leaves it for k_pcr_weigh
static G1A through_affine(const G1A& p) {
  std::vector<int32_t> col(2 * NL);
  pcr_store_affine(col.data(), 1, p);
  return pcr_load_affine(col.data(), 1);
}
static G1A load_g1(const std::vector<uint8_t>& p) {
  bool ok;
  const G1A a = g1_decode(p.data(), ok);
  if (!ok || a.inf) { std::fprintf(stderr, "not an affine point\n"); std::exit(3); }
  return through_affine(a);
}
// a result as the kernels leave it and as k_g1_seg_sum reads it back
static void print_stored(const G1P& p) {
  std::vector<int32_t> col(3 * NL);
  agr_store_point(col.data(), 1, p);
  uint8_t enc[64];
  g1_encode(enc, g1_to_affine(agr_load_point(col.data(), 1)));
  print_hex(enc, 64);
}
// k_g2_prepare's validity byte of a key
static uint8_t key_ok_of(const uint8_t* g2) {
  bool okd;
  const G2A q = g2_decode(g2, okd);
  if (!(okd && !q.inf && g2_on_curve(q))) return 0;
  return g2_torsion_free(q) ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s <command file>\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::string cmd;
  while (in >> cmd) {
    if (cmd == "digest") {
      const std::vector<uint8_t> dg = blob(in);
      const AgrWeight w = agr_weight_of_digest(dg.data());
      std::printf("digest %u %u\n", w.a, w.b);
    } else if (cmd == "weight") {
      const std::vector<uint8_t> seed = blob(in);
      uint64_t g; in >> g;
      const AgrWeight w = pcr_weight(seed.data(), g);
      std::printf("weight %u %u\n", w.a, w.b);
    } else if (cmd == "mul") {
      uint32_t a, b; in >> a >> b;
      const std::vector<uint8_t> p = blob(in);
      std::printf("mul "); print_stored(pcr_mul_glv32(load_g1(p), a, b)); std::printf("\n");
    } else if (cmd == "mul2") {
      uint32_t a, b, c, d;
      in >> a >> b;
      const std::vector<uint8_t> p = blob(in);
      in >> c >> d;
      const std::vector<uint8_t> q = blob(in);
      G1P rp, rq;
      pcr_mul_glv32_x2(load_g1(p), AgrWeight{a, b}, load_g1(q), AgrWeight{c, d}, rp, rq);
      std::printf("mul2 "); print_stored(rp); std::printf(" "); print_stored(rq); std::printf("\n");
    } else if (cmd == "pair") {
      const std::vector<uint8_t> g1 = blob(in), g2 = blob(in);
      G1A p;
      const uint8_t f = pcr_pair(g1.data(), g2.data(), key_ok_of(g2.data()), p);
      std::printf("pair %d %d\n", (f & PCR_OK) ? 1 : 0, (f & PCR_SKIP) ? 1 : 0);
    } else if (cmd == "lane") {
      const std::vector<uint8_t> g1 = blob(in), g2 = blob(in);
      uint32_t a, b; int elig; in >> a >> b >> elig;
      G1A p;
      const uint8_t f = pcr_pair(g1.data(), g2.data(), key_ok_of(g2.data()), p);
      G1P r0, r1;
      const G1A q = through_affine(p);
      pcr_mul_glv32_x2(q, AgrWeight{a, b}, q, AgrWeight{a, b}, r0, r1);
      std::printf("lane "); print_stored(proj_select((elig != 0) & !(f & PCR_SKIP), r0, proj_identity<Fp>())); std::printf("\n");
    } else if (cmd == "eligible") {
      size_t n; in >> n;
      const std::vector<uint8_t> flag = nums<uint8_t>(in, n);
      std::printf("eligible %d\n", pcr_eligible(flag.data(), 0, (uint32_t)n) ? 1 : 0);
    } else if (cmd == "round1") {
      size_t N, u, mx; in >> N >> u >> mx;
      std::printf("round1 %d\n", pcr_round1(N, u, mx) ? 1 : 0);
    } else if (cmd == "consts") {
      std::printf("consts %zu %zu %zu\n", PCR_SMAX, PCR_MERGE_GAP, AGR_MAX_SEGMENTS);
    } else if (cmd == "segments") {
      size_t setting, smax, N, u, G; in >> setting >> smax >> N >> u >> G;
      std::printf("segments %zu\n", agr_segments(setting, smax, N, u, G));
    } else if (cmd == "cut") {
      size_t G, S; in >> G >> S;
      std::vector<uint32_t> bound, seg_of;
      agr_cut(G, S, bound, seg_of);
      std::printf("cut");
      for (uint32_t x : bound) std::printf(" %u", x);
      for (uint32_t x : seg_of) std::printf(" %u", x);
      std::printf("\n");
    } else if (cmd == "ranges") {
      size_t S; in >> S;
      const std::vector<uint32_t> bound = nums<uint32_t>(in, S + 1);
      const std::vector<uint8_t> pass = nums<uint8_t>(in, S);
      size_t G; in >> G;
      const std::vector<uint8_t> elig = nums<uint8_t>(in, G);
      const std::vector<uint64_t> off = nums<uint64_t>(in, G + 1);
      size_t gap; in >> gap;
      std::vector<std::pair<size_t, size_t>> out;
      size_t eligible;
      agr_failed_ranges(bound, pass.data(), elig.data(), off.data(), gap, out, &eligible);
      std::printf("ranges %zu %zu", eligible, out.size());
      for (const auto& r : out) std::printf(" %zu %zu", r.first, r.second);
      std::printf("\n");
    } else { std::fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
  }
  return 0;
}
