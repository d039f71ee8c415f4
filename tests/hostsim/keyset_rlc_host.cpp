// keyset_rlc_host.cpp -- the lane functions of csrc/keyset_rlc.h (key-set FastAggregateVerify by random linear combination per
// message) and the plain C++ of csrc/keyset_rlc_plan.h compiled for the host with -DBN_CHECK, for tests/test_keyset_rlc_host.py.
// A STAND-ALONE program: it reads commands from the file named on its command line and prints one line of results per command, so
// a host sanitizer build of it (-fsanitize=address,undefined) runs as it is.  TEST TOOL ONLY.
//   plan     C n_groups msg(hex) x n_groups            -> n_classes n_chunks n_levels n_multi items_max, order, pos, chunk_of, multi,
//                                                         rep (per class), per chunk start len class, per level its run count and
//                                                         the runs' start len
//   mulg2    r pk(hex, 128 bytes)                      -> the encoding of [r] P by ksr_mul_u64
//   mulg1    r sig(hex, 64 bytes)                      -> likewise in G1
//   digest   dg(hex, 32 bytes)                         -> ksr_weight_of_digest
//   weight   seed(hex) g sig(hex)                      -> ksr_weight
//   rowvalid n_keys row(hex) skip(words) valid(words)  -> ksr_row_valid
//   sigok    sig(hex)                                  -> ksr_sig_ok
//   elig     row_ok row_valid sig_ok sum_identity      -> ksr_eligible
//   chunk    n_members (elig r pk(hex)) x n_members    -> the lane of k_ksr_chunks on the G2 side: the members' weighted points summed,
//                                                         stored as the kernels store them; eligible count, "is the identity", and the
//                                                         state for a G1 sum that is not the identity
// Blobs are hex strings, "-" for an empty one; numbers are decimal.
#include "../../bls-bn254_amd/csrc/keyset_rlc.h"
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
static G2P load_pk(const std::vector<uint8_t>& pk) {
  bool ok;
  const G2A a = g2_decode(pk.data(), ok);
  if (!ok) { std::fprintf(stderr, "a key does not decode\n"); std::exit(3); }
  return proj_from_affine(a);
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s <command file>\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::string cmd;
  while (in >> cmd) {
    if (cmd == "plan") {
      size_t C, n; in >> C >> n;
      std::vector<uint8_t> msgs;
      std::vector<uint64_t> off(1, 0);
      for (size_t g = 0; g < n; ++g) { const std::vector<uint8_t> m = blob(in); msgs.insert(msgs.end(), m.begin(), m.end()); off.push_back(msgs.size()); }
      KsrPlan P;
      std::vector<uint32_t> start, len;
      if (!ksr_plan(msgs.empty() ? nullptr : msgs.data(), off.data(), n, C, P, start, len)) return 3;
      std::printf("plan %zu %zu %zu %zu %zu", P.rep.size(), P.chunks.size(), P.levels.size(), P.n_multi, P.items_max);
      for (const auto* v : {&P.order, &P.pos, &P.chunk_of}) for (uint32_t x : *v) std::printf(" %u", x);
      for (uint8_t x : P.multi) std::printf(" %u", x);
      for (uint32_t x : P.rep) std::printf(" %u", x);
      for (const KsrChunk& c : P.chunks) std::printf(" %u %u %u", c.start, c.len, c.cls);
      for (const SegLevel& lv : P.levels) {
        std::printf(" %zu", lv.count);
        for (size_t r = 0; r < lv.count; ++r) std::printf(" %u %u", start[lv.first + r], len[lv.first + r]);
      }
      std::printf("\n");
    } else if (cmd == "mulg2") {
      uint64_t r; in >> r;
      const std::vector<uint8_t> pk = blob(in);
      uint8_t enc[128];
      g2_encode(enc, g2_to_affine(ksr_mul_u64(load_pk(pk), r)));
      std::printf("mulg2 "); print_hex(enc, 128); std::printf("\n");
    } else if (cmd == "mulg1") {
      uint64_t r; in >> r;
      const std::vector<uint8_t> sig = blob(in);
      bool ok;
      const G1A a = g1_decode(sig.data(), ok);
      uint8_t enc[64];
      g1_encode(enc, g1_to_affine(ksr_mul_u64(proj_from_affine(a), r)));
      std::printf("mulg1 "); print_hex(enc, 64); std::printf("\n");
    } else if (cmd == "digest") {
      const std::vector<uint8_t> dg = blob(in);
      std::printf("digest %" PRIu64 "\n", ksr_weight_of_digest(dg.data()));
    } else if (cmd == "weight") {
      const std::vector<uint8_t> seed = blob(in);
      uint64_t g; in >> g;
      const std::vector<uint8_t> sig = blob(in);
      std::printf("weight %" PRIu64 "\n", ksr_weight(seed.data(), g, sig.data()));
    } else if (cmd == "rowvalid") {
      uint32_t n; in >> n;
      const std::vector<uint8_t> row = blob(in);
      const std::vector<uint32_t> skip = nums<uint32_t>(in, ks_words(n)), valid = nums<uint32_t>(in, ks_words(n));
      std::printf("rowvalid %d\n", ksr_row_valid(row.data(), n, skip.data(), valid.data()) ? 1 : 0);
    } else if (cmd == "sigok") {
      const std::vector<uint8_t> sig = blob(in);
      G1A p;
      std::printf("sigok %d\n", ksr_sig_ok(sig.data(), p) ? 1 : 0);
    } else if (cmd == "elig") {
      const std::vector<int> v = nums<int>(in, 4);
      std::printf("elig %d\n", ksr_eligible(v[0] != 0, v[1] != 0, v[2] != 0, v[3] != 0) ? 1 : 0);
    } else if (cmd == "chunk") {
      size_t m; in >> m;
      G2P sum = proj_identity<Fp2>();
      uint32_t eligible = 0;
      for (size_t j = 0; j < m; ++j) {
        int e; uint64_t r; in >> e >> r;
        const std::vector<uint8_t> pk = blob(in);
        // k_ksr_weigh_g2: an ineligible member stores the identity; then one run of k_g2_seg_sum
        const G2P B = e ? ksr_mul_u64(load_pk(pk), r) : proj_identity<Fp2>();
        std::vector<int32_t> col(6 * NL);
        ks_store_point(col.data(), 1, B);
        sum = proj_add(sum, ks_load_point(col.data(), 1));
        eligible += e ? 1 : 0;
      }
      std::vector<int32_t> col(6 * NL);
      ks_store_point(col.data(), 1, sum);
      const bool ident = ksr_is_identity(col.data(), 1);
      std::printf("chunk %u %d %u\n", eligible, ident ? 1 : 0, ksr_chunk_state(eligible, false, ident));
    } else { std::fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
  }
  return 0;
}
