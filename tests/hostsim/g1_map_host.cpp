// g1_map_host.cpp -- lane_hash_tai.h (the lane functions of k_hash_tai.hip: the start value, the search, the point) compiled for
// the host with -DBN_CHECK, so the interval checks run over the whole new path.  As a shared object the functions below are
// compared byte for byte with tests/g1_map_support.py by tests/test_g1_map_host.py -- once as the library has it and once with
// -DTAI_CAP=4, where a digest with a long run reaches the cap; as a stand-alone program (main below; built with the address and
// undefined-behaviour sanitizers) it runs the same functions over exact-size buffers of every length 0 .. 100 and checks what
// needs no model: the point is on the curve, its x is x0 + k, and the run is what stepping by hand finds.
// TEST TOOL ONLY: the product has no CPU path.
#include "../../bls-bn254_amd/csrc/lane_hash_tai.h"
#include <cstdio>
#include <cstring>
#include <vector>

using namespace bn;

extern "C" {

int hs_tai_cap() { return (int)TAI_CAP; }
void hs_tai_digest(uint32_t xid, const uint8_t* msg, size_t len, uint8_t* out) { tai_plain_digest(xid, out, msg, len); }
void hs_tai_x0(uint32_t map, uint32_t xid, const uint8_t* msg, size_t len, uint8_t* out) { fp_to_be(out, tai_x0(map, xid, msg, len)); }
// the composition of the kernels: 64 bytes x || y, (0, 0) at the cap; returns the candidates skipped (TAI_CAP at the cap)
int hs_tai_hash_to_g1(uint32_t map, uint32_t xid, const uint8_t* msg, size_t len, uint8_t* out) {
  Fp x = tai_x0(map, xid, msg, len);
  uint32_t k;
  const bool found = tai_search(x, k);
  g1_encode(out, tai_point(x, found));
  return (int)k;
}
void hs_tai_lane(uint32_t map, uint32_t xid, const uint8_t* msg, size_t len, uint8_t* out) { g1_encode(out, lane_hash_to_g1_tai(map, xid, msg, len)); }

}  // extern "C"

namespace {
int fails = 0;
void expect(bool ok, const char* what, size_t at) { if (!ok) { std::fprintf(stderr, "FAIL %s (%zu)\n", what, at); ++fails; } }
}  // namespace

int main() {
  for (uint32_t map : {(uint32_t)G1MAP_TAI_DIGEST, (uint32_t)G1MAP_TAI_HASH}) {
    for (size_t len = 0; len <= 100; ++len) {
      std::vector<uint8_t> msg(len);                                   // exactly as long as what is read
      for (size_t i = 0; i < len; ++i) msg[i] = (uint8_t)(37 * i + 11 * len + map);
      const uint32_t xid = (uint32_t)(len % EXPAND_COUNT);
      std::vector<uint8_t> out(64), again(64), x0b(32);
      const int k = hs_tai_hash_to_g1(map, xid, msg.data(), len, out.data());
      hs_tai_lane(map, xid, msg.data(), len, again.data());
      expect(out == again, "the lane function is the composition", len);
      if (k >= (int)TAI_CAP) { expect(out == std::vector<uint8_t>(64, 0), "(0, 0) at the cap", len); continue; }
      bool okx, oky;
      G1A p; p.x = fp_from_be(out.data(), okx); p.y = fp_from_be(out.data() + 32, oky); p.inf = false;
      expect(okx && oky && g1_on_curve(p), "on the curve", len);
      Fp x = tai_x0(map, xid, msg.data(), len);
      int steps = 0;
      while (!fp_is_square(tai_rhs(x)) && steps < (int)TAI_CAP) { x = tai_offset(x, 1); ++steps; }
      expect(steps == k && fp_eq(x, p.x), "the run stepped by hand", len);
    }
  }
  if (fails) return 1;
  std::printf("g1_map_host ok\n");
  return 0;
}
