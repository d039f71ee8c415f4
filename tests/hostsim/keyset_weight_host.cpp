// keyset_weight_host.cpp -- the lane functions of csrc/keyset_weight.h (stake weights over a registered key set selected by
// bitmaps) and the plain C++ of csrc/keyset_weight_plan.h compiled for the host, for tests/test_keyset_weight_host.py.  A
// STAND-ALONE program: it reads commands from the file named on its command line and prints one line of results per command, so
// a host sanitizer build of it (-fsanitize=address,undefined) runs as it is.  A wave of k_ks_weight is run as 64 lane states:
// every lane's accumulators first, then the six rounds of the reduction with the two 32-bit halves carried from lane to lane by
// this harness, standing in for the shuffles (a lane past the wave's end reads its own value, as the hardware gives it).
// TEST TOOL ONLY.
//   major   n_keys n_cols weights(n_cols*n_keys)                                 -> the table as the device holds it, key-major
//   weight  n_keys n_cols n_groups g_lo m valid(hex, a byte per key) weights(...) rows(hex)
//                                                                                -> the m x n_cols sums of groups g_lo .. g_lo + m
//   fit     n_keys n_cols weights(...)                                           -> the first overflowing column or -1
//   plan    n_groups chunk                                                       -> groups per launch, launches
//   quorum  n_groups n_cols row_bytes min(n_cols) weights(n_groups*n_cols) off(n_groups+1) rows(hex) sigs(hex) msgs(hex, from byte 0)
//           sub_bits(hex)  -> count, the reaching groups, the sub-call's offsets, rows, sigs, msgs (hex) and the scattered bitmap (hex)
// Blobs are hex strings, "-" for an empty one; numbers are decimal.
#include "../../bls-bn254_amd/csrc/keyset_weight.h"
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
static std::vector<uint64_t> nums(std::istream& in, size_t n) {
  std::vector<uint64_t> v(n);
  for (size_t i = 0; i < n; ++i) in >> v[i];
  return v;
}
static void put_hex(const std::vector<uint8_t>& v) {
  if (v.empty()) std::printf(" -");
  else { std::printf(" "); for (uint8_t b : v) std::printf("%02x", b); }
}

// the KeyValidate bits by words, as the registration packs them
static std::vector<uint32_t> pack_words(const std::vector<uint8_t>& valid, uint32_t n_keys) {
  std::vector<uint32_t> v(ks_words(n_keys), 0);
  for (uint32_t i = 0; i < n_keys; ++i)
    if (valid[i]) v[i >> 5] |= 1u << (i & 31);
  return v;
}
// k_ks_weight for one group
static void wave(const uint8_t* row, uint32_t n_keys, const uint32_t* vwords, const uint64_t* tab, uint32_t n_cols, uint64_t* out) {
  KwAcc a[KW_WAVE];
  for (uint32_t l = 0; l < KW_WAVE; ++l) a[l] = kw_lane_sum(row, n_keys, l, vwords, tab, n_cols);
  for (uint32_t d = KW_WAVE / 2; d; d >>= 1)
    for (uint32_t q = 0; q < n_cols; ++q) {
      uint32_t lo[KW_WAVE], hi[KW_WAVE];
      for (uint32_t l = 0; l < KW_WAVE; ++l) {           // every lane's read before any lane's write
        const uint32_t src = l + d < KW_WAVE ? l + d : l;
        lo[l] = kw_lo(a[src].v[q]); hi[l] = kw_hi(a[src].v[q]);
      }
      for (uint32_t l = 0; l < KW_WAVE; ++l) a[l].v[q] += kw_join(lo[l], hi[l]);
    }
  for (uint32_t q = 0; q < n_cols; ++q) out[q] = a[0].v[q];
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s <command file>\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::string cmd;
  while (in >> cmd) {
    if (cmd == "major") {
      size_t n, nc; in >> n >> nc;
      const std::vector<uint64_t> w = nums(in, n * nc);
      std::vector<uint64_t> tab;
      kw_key_major(w.data(), n, nc, tab);
      std::printf("major");
      for (uint64_t v : tab) std::printf(" %" PRIu64, v);
      std::printf("\n");
    } else if (cmd == "weight") {
      uint32_t n, nc; size_t ng, g_lo, m; in >> n >> nc >> ng >> g_lo >> m;
      const std::vector<uint8_t> valid = blob(in);
      const std::vector<uint64_t> w = nums(in, (size_t)n * nc);
      const std::vector<uint8_t> rows = blob(in);
      const std::vector<uint32_t> vwords = pack_words(valid, n);
      std::vector<uint64_t> tab;
      kw_key_major(w.data(), n, nc, tab);
      std::vector<uint64_t> out(ng * nc, 0xeeeeeeeeeeeeeeeeull);
      for (size_t g = g_lo; g < g_lo + m; ++g) wave(rows.data() + g * ks_row_bytes(n), n, vwords.data(), tab.data(), nc, out.data() + g * nc);
      std::printf("weight");
      for (size_t i = g_lo * nc; i < (g_lo + m) * nc; ++i) std::printf(" %" PRIu64, out[i]);
      std::printf("\n");
    } else if (cmd == "fit") {
      size_t n, nc; in >> n >> nc;
      const std::vector<uint64_t> w = nums(in, n * nc);
      std::printf("fit %d\n", kw_overflowing_column(w.data(), n, nc));
    } else if (cmd == "plan") {
      size_t ng, chunk; in >> ng >> chunk;
      std::printf("plan %zu %zu\n", kw_launch_groups(chunk), kw_launches(ng, chunk));
    } else if (cmd == "quorum") {
      size_t ng, nc, rb; in >> ng >> nc >> rb;
      const std::vector<uint64_t> minw = nums(in, nc), w = nums(in, ng * nc), off = nums(in, ng + 1);
      const std::vector<uint8_t> rows = blob(in), sigs = blob(in), msgs = blob(in), sub_bits = blob(in);
      std::vector<size_t> reach;
      kw_reaching(w.data(), minw.data(), ng, nc, reach);
      KwRepack r;
      kw_repack(reach, rows.data(), rb, msgs.empty() ? nullptr : msgs.data(), off.data(), sigs.data(), r);
      std::vector<uint8_t> bm((ng + 7) / 8, 0);
      kw_scatter_bits(reach, sub_bits.data(), bm.data());
      std::printf("quorum %zu", reach.size());
      for (size_t g : reach) std::printf(" %zu", g);
      for (uint64_t o : r.off) std::printf(" %" PRIu64, o);
      put_hex(r.rows); put_hex(r.sigs); put_hex(r.msgs); put_hex(bm);
      std::printf("\n");
    } else { std::fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
  }
  return 0;
}
