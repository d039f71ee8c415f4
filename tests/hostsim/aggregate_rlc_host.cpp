// aggregate_rlc_host.cpp -- the lane functions of csrc/aggregate_rlc.h (aggregate verify over ragged groups by random linear
// combination) and the plain C++ of csrc/aggregate_rlc_plan.h compiled for the host with -DBN_CHECK, for
// tests/test_aggregate_rlc_host.py.  A STAND-ALONE program: it reads commands from the file named on its command line and prints
// one line of results per command, so a host sanitizer build of it (-fsanitize=address,undefined) runs as it is.  TEST TOOL ONLY.
//   digest   dg(hex, 32 bytes)                          -> a b of agr_weight_of_digest
//   weight   seed(hex) g sig(hex)                       -> a b of agr_weight
//   mul      a b p(hex, 64 bytes)                       -> the encoding of [a + b lambda] P by agr_mul_glv32
//   mul2     a b p(hex) c d q(hex)                      -> the two encodings by agr_mul_glv32_x2, through the stored layout
//   sigok    sig(hex)                                   -> agr_sig_ok
//   pairs    G off x (G + 1)                            -> agr_pair_groups
//   repeat   N u max_keys                               -> agr_keys_repeat
//   segments setting s_max N u G                        -> agr_segments
//   cut      G S                                        -> the S + 1 bounds, then the G segments
//   ranges   S bound x (S + 1) pass x S G elig x G off x (G + 1) merge_gap -> eligible n_ranges, then first second per range
// Blobs are hex strings, "-" for an empty one; numbers are decimal.
#include "../../bls-bn254_amd/csrc/aggregate_rlc.h"
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
  if (s == "-") return v;
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
static G1P load_g1(const std::vector<uint8_t>& p) {
  bool ok;
  const G1A a = g1_decode(p.data(), ok);
  if (!ok) { std::fprintf(stderr, "a point does not decode\n"); std::exit(3); }
  return proj_from_affine(a);
}
// a result as the kernels leave it and as k_g1_seg_sum reads it back
static void print_stored(const G1P& p) {
  std::vector<int32_t> col(3 * NL);
  agr_store_point(col.data(), 1, p);
  uint8_t enc[64];
  g1_encode(enc, g1_to_affine(agr_load_point(col.data(), 1)));
  print_hex(enc, 64);
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
      const std::vector<uint8_t> sig = blob(in);
      const AgrWeight w = agr_weight(seed.data(), g, sig.data());
      std::printf("weight %u %u\n", w.a, w.b);
    } else if (cmd == "mul") {
      uint32_t a, b; in >> a >> b;
      const std::vector<uint8_t> p = blob(in);
      std::printf("mul "); print_stored(agr_mul_glv32(load_g1(p), a, b)); std::printf("\n");
    } else if (cmd == "mul2") {
      uint32_t a, b, c, d;
      in >> a >> b;
      const std::vector<uint8_t> p = blob(in);
      in >> c >> d;
      const std::vector<uint8_t> q = blob(in);
      G1P rp, rq;
      agr_mul_glv32_x2(load_g1(p), AgrWeight{a, b}, load_g1(q), AgrWeight{c, d}, rp, rq);
      std::printf("mul2 "); print_stored(rp); std::printf(" "); print_stored(rq); std::printf("\n");
    } else if (cmd == "sigok") {
      const std::vector<uint8_t> sig = blob(in);
      G1A p;
      std::printf("sigok %d\n", agr_sig_ok(sig.data(), p) ? 1 : 0);
    } else if (cmd == "pairs") {
      size_t G; in >> G;
      const std::vector<uint64_t> off = nums<uint64_t>(in, G + 1);
      std::vector<uint32_t> gidx;
      agr_pair_groups(off.data(), G, gidx);
      std::printf("pairs");
      for (uint32_t x : gidx) std::printf(" %u", x);
      std::printf("\n");
    } else if (cmd == "repeat") {
      size_t N, u, mx; in >> N >> u >> mx;
      std::printf("repeat %d\n", agr_keys_repeat(N, u, mx) ? 1 : 0);
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
