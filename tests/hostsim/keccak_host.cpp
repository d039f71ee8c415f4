// keccak_host.cpp -- keccak.h (the permutation, the byte-wise sponge, the expanders and their dispatcher, the oversize-DST rule)
// and lane_hash_x.h (the lane functions of k_hash_keccak.hip) compiled for the host with -DBN_CHECK.  As a shared object the
// functions below are compared byte for byte with tests/expander_support.py by tests/test_keccak_host.py; as a stand-alone
// program (main below; built with the address and undefined-behaviour sanitizers) it runs keccak.h -- all of the feature that the
// product's host side executes (stage_dst's oversize rule) -- over every length and checks what needs no model: the two published
// Keccak-256 digests, the Z_pad constant against the permutation of zero, byte-wise against split absorption and squeezing.
// The sanitized build leaves the lane functions out (KC_LANES): they are device code, the field arithmetic behind them shifts
// signed limbs left (fp29.h fp_lc), which the sanitizer reports, and instrumenting the curve code takes minutes to compile.
// TEST TOOL ONLY: the product has no CPU path.
#if defined(__SANITIZE_ADDRESS__)
#include "../../bls-bn254_amd/csrc/keccak.h"
#else
#define KC_LANES
#include "../../bls-bn254_amd/csrc/lane_hash_x.h"
#endif
#include <cstdio>
#include <cstring>
#include <vector>

using namespace bn;

extern "C" {

void hs_kc_f(uint64_t* st) { keccak_f(st); }
void hs_kc_zpad_state(uint64_t* out) { Keccak s; keccak_init_zpad(s); std::memcpy(out, s.a, sizeof s.a); }
// out[0..n) = the sponge at `rate` under `domain` of msg: Keccak-256 (136, 0x01), SHA3-256 (136, 0x06), SHAKE-128 / -256 (168 / 136, 0x1F)
void hs_kc_hash(const uint8_t* msg, size_t len, uint32_t rate, int domain, uint8_t* out, size_t n) { keccak_hash(out, n, msg, len, rate, (uint8_t)domain); }
void hs_kc_expand(uint32_t xid, const uint8_t* msg, size_t len, const uint8_t* dst, uint32_t dst_len, uint8_t* out, uint32_t n) {
  expand_message(xid, out, n, msg, len, dst, dst_len);
}
void hs_kc_oversize_dst(uint32_t xid, const uint8_t* dst, size_t dst_len, uint8_t* out) { oversize_dst(xid, out, dst, dst_len); }
#ifdef KC_LANES
// the compositions of the kernels (dst_len <= 255: the host stages an oversize tag through hs_kc_oversize_dst's function)
void hs_kc_hash_to_g1(uint32_t xid, const uint8_t* msg, size_t len, const uint8_t* dst, uint32_t dst_len, int mode, uint8_t* out) {
  const G1A h = mode == 2 ? lane_encode_to_g1_x(xid, msg, len, dst, dst_len)
              : mode == 3 ? g1_to_affine(lane_hash_to_g1_proj_x(xid, msg, len, dst, dst_len)) : lane_hash_to_g1_x(xid, msg, len, dst, dst_len);
  g1_encode(out, h);
}
void hs_kc_hash_to_g2(uint32_t xid, const uint8_t* msg, size_t len, const uint8_t* dst, uint32_t dst_len, int ro, uint8_t* out) {
  g2_encode(out, lane_hash_to_g2_x(xid, msg, len, dst, dst_len, ro != 0));
}
void hs_kc_hash_to_scalar(uint32_t xid, const uint8_t* msg, size_t len, const uint8_t* dst, uint32_t dst_len, uint8_t* out) {
  fr_to_be(out, lane_hash_to_scalar_x(xid, msg, len, dst, dst_len));
}
#endif

}  // extern "C"

namespace {
int fails = 0;
void expect(bool ok, const char* what) { if (!ok) { std::fprintf(stderr, "FAIL %s\n", what); ++fails; } }
void from_hex(const char* hex, uint8_t* out, size_t n) {
  for (size_t i = 0; i < n; ++i) { unsigned v; std::sscanf(hex + 2 * i, "%2x", &v); out[i] = (uint8_t)v; }
}
}  // namespace

int main() {
  uint8_t want[32], got[200];
  from_hex("c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470", want, 32);
  keccak_hash(got, 32, nullptr, 0, KECCAK_RATE_256, KECCAK_DOMAIN_KECCAK);
  expect(std::memcmp(got, want, 32) == 0, "Keccak-256 of the empty string");
  from_hex("4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45", want, 32);
  keccak_hash(got, 32, (const uint8_t*)"abc", 3, KECCAK_RATE_256, KECCAK_DOMAIN_KECCAK);
  expect(std::memcmp(got, want, 32) == 0, "Keccak-256 of abc");
  uint64_t z[25] = {0}, zp[25];
  keccak_f(z); hs_kc_zpad_state(zp);
  expect(std::memcmp(z, zp, sizeof z) == 0, "Z_pad constant == Keccak-f(0)");
  // every length 0 .. 400 at both rates, each buffer exactly as long as what is read or written: absorbed in one piece and in two,
  // squeezed in one piece and in three, must agree
  for (size_t len = 0; len <= 400; ++len) {
    std::vector<uint8_t> msg(len);
    for (size_t i = 0; i < len; ++i) msg[i] = (uint8_t)(31 * i + len);
    for (uint32_t rate : {(uint32_t)KECCAK_RATE_256, (uint32_t)KECCAK_RATE_128}) {
      std::vector<uint8_t> a(200), b(200);
      keccak_hash(a.data(), 200, msg.data(), len, rate, KECCAK_DOMAIN_SHAKE);
      Keccak s; keccak_init(s, rate);
      keccak_update(s, msg.data(), len / 3); keccak_update(s, msg.data() + len / 3, len - len / 3);
      keccak_finish(s, KECCAK_DOMAIN_SHAKE);
      keccak_squeeze(s, b.data(), 7); keccak_squeeze(s, b.data() + 7, 161); keccak_squeeze(s, b.data() + 168, 32);
      expect(a == b, "split absorb / squeeze");
    }
  }
  // the expanders and the lane functions over exact-size buffers, every id, the DST lengths at and around the limit
  for (uint32_t xid = 0; xid < EXPAND_COUNT; ++xid) {
    for (size_t dl : {(size_t)1, (size_t)43, (size_t)255, (size_t)256, (size_t)300}) {
      std::vector<uint8_t> dst(dl, (uint8_t)('A' + xid)), eff(dst);
      if (dl > 255) { eff.assign(32, 0); oversize_dst(xid, eff.data(), dst.data(), dl); }
      for (size_t len : {(size_t)0, (size_t)1, (size_t)135, (size_t)136, (size_t)167, (size_t)168, (size_t)1000}) {
        std::vector<uint8_t> msg(len, (uint8_t)len);
        for (uint32_t n : {48u, 96u, 192u}) {
          std::vector<uint8_t> out(n), again(n);
          expand_message(xid, out.data(), n, msg.data(), len, eff.data(), (uint32_t)eff.size());
          expand_message(xid, again.data(), n, msg.data(), len, eff.data(), (uint32_t)eff.size());
          expect(out == again, "expand_message is a function of its inputs");
        }
      }
#ifdef KC_LANES
      uint8_t p1[64], p3[64], sc[32];
      hs_kc_hash_to_g1(xid, (const uint8_t*)"host", 4, eff.data(), (uint32_t)eff.size(), 1, p1);
      hs_kc_hash_to_g1(xid, (const uint8_t*)"host", 4, eff.data(), (uint32_t)eff.size(), 3, p3);
      expect(std::memcmp(p1, p3, 64) == 0, "affine and homogeneous hash agree");
      hs_kc_hash_to_scalar(xid, (const uint8_t*)"host", 4, eff.data(), (uint32_t)eff.size(), sc);
#endif
    }
  }
  if (fails) return 1;
  std::printf("keccak_host ok\n");
  return 0;
}
