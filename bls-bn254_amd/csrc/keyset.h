// keyset.h -- what ONE lane does in the sums over a REGISTERED key set selected by bitmaps (k_keyset.hip, host_keyset.hip).
// A key set holds n_keys G2 keys once: affine, limb-major rows (36 limbs x n_keys), and per 32-key WORD (W = ceil(n_keys / 32))
// a `bad` word (the key does not decode or is off the curve) and a `skip` word (bad, or the identity: never added), plus the
// total T = sum of the non-skipped keys.  A call brings n_groups ROWS of ceil(n_keys / 8) bytes, bit i (LSB-first) = key i
// signed.  Groups are uniform -- every group spans the same W words -- so every lane derives its run from its index:
//   ks_count        a row's popcount -> flip = 2 popcount > n_keys (sum the UNSELECTED keys and take T - that), ok = no selected
//                   key is bad
//   ks_word_mask    the keys a lane adds for one word of its row: (flip ? ~word : word) & ~skip & tail
//   ks_word_sum     their sum by mixed additions out of the word's 32 staged keys ([limb][32])
//   ks_group_run    one lane of a reduction pass: the sum of up to KS_RUN partials of one group, items laid out WORD-major
//                   (item w G + g, G = groups of the launch), so stores and the next pass's loads are coalesced across groups
//   ks_finish       the last pass: U -> flip ? T + (-U) : U, the identity for a row that selects a bad key
// tests/hostsim/keyset_host.cpp runs the same functions on the host with -DBN_CHECK against a Python model.  They are not a
// CPU fallback: nothing in the product's host path calls them.
#pragma once
#include "lane_ops.h"

namespace bn {

constexpr uint32_t KS_RUN = 16;                  // partials per lane of a reduction pass
constexpr int KS_AFF_LIMBS = 4 * NL;             // x.c0, x.c1, y.c0, y.c1

BN_INL uint32_t ks_words(uint32_t n_keys) { return (n_keys + 31) / 32; }
BN_INL uint32_t ks_row_bytes(uint32_t n_keys) { return (n_keys + 7) / 8; }
// the bits of word w that name a key
BN_INL uint32_t ks_tail_mask(uint32_t n_keys, uint32_t w) {
  const uint32_t left = n_keys - 32 * w;
  return left >= 32 ? 0xffffffffu : (1u << left) - 1u;
}
// word w of a row, assembled from bytes (rows need no alignment; bytes past the row read as 0)
BN_INL uint32_t ks_row_word(const uint8_t* row, uint32_t row_bytes, uint32_t w) {
  uint32_t v = 0;
  for (uint32_t b = 0; b < 4; ++b) {
    const uint32_t i = 4 * w + b;
    v |= (i < row_bytes ? (uint32_t)row[i] : 0u) << (8 * b);
  }
  return v;
}
BN_INL uint32_t ks_popc(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popc(v);
#else
  return (uint32_t)__builtin_popcount(v);
#endif
}
BN_INL uint32_t ks_ctz(uint32_t v) {             // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)(__ffs((int)v) - 1);
#else
  return (uint32_t)__builtin_ctz(v);
#endif
}

struct KsCount { bool flip, ok; };
BN_INL KsCount ks_count(const uint8_t* row, uint32_t n_keys, const uint32_t* bad) {
  const uint32_t W = ks_words(n_keys), rb = ks_row_bytes(n_keys);
  uint32_t pop = 0, hit = 0;
#pragma unroll 4                                 // one lane per group is bound by the latency of the row's byte loads: four words in flight per trip
  for (uint32_t w = 0; w < W; ++w) {
    const uint32_t v = ks_row_word(row, rb, w) & ks_tail_mask(n_keys, w);
    pop += ks_popc(v);
    hit |= v & bad[w];
  }
  return {2 * pop > n_keys, hit == 0};
}
BN_INL uint32_t ks_word_mask(uint32_t word, bool flip, uint32_t skip, uint32_t tail) { return (flip ? ~word : word) & ~skip & tail; }

// registration with proofs of possession: bit i of mask (LSB-first) = the proof of key i verifies; no mask: every key passes
BN_INL bool ks_mask_bit(const uint8_t* mask, uint32_t i) { return mask ? ((mask[i >> 3] >> (i & 7)) & 1u) != 0 : true; }
// an encoding that does not decode (every coordinate >= p) over a staged key; the staging buffer is 16-byte aligned
BN_INL void ks_blank_enc(uint8_t* pk) {
  uint32_t* w = (uint32_t*)pk;
  for (int j = 0; j < 32; ++j) w[j] = 0xffffffffu;
}
// registration: a key's affine coordinates and its two bits.  A skipped key's row is never read back.
struct KsKey { G2A p; bool bad, skip; };
BN_FUNC KsKey ks_register(const uint8_t* pk) {
  BN_CTX;
  bool okd;
  KsKey k;
  k.p = g2_decode(pk, okd);
  k.bad = !(okd & g2_on_curve(k.p));
  k.skip = k.bad | k.p.inf;
  return k;
}
BN_FUNC void ks_store_aff(int32_t* ws, size_t stride, const G2A& p) {
  store_fp(ws, stride, p.x.c0); store_fp(ws + NL * stride, stride, p.x.c1);
  store_fp(ws + 2 * NL * stride, stride, p.y.c0); store_fp(ws + 3 * NL * stride, stride, p.y.c1);
}
BN_FUNC G2A ks_load_aff(const int32_t* ws, size_t stride) {
  G2A p;
  p.x = {load_fp(ws, stride), load_fp(ws + NL * stride, stride)};
  p.y = {load_fp(ws + 2 * NL * stride, stride), load_fp(ws + 3 * NL * stride, stride)};
  p.inf = false;
  return p;
}
BN_FUNC void ks_store_point(int32_t* ws, size_t stride, const G2P& p) {
  store_fp(ws, stride, p.x.c0); store_fp(ws + NL * stride, stride, p.x.c1);
  store_fp(ws + 2 * NL * stride, stride, p.y.c0); store_fp(ws + 3 * NL * stride, stride, p.y.c1);
  store_fp(ws + 4 * NL * stride, stride, p.z.c0); store_fp(ws + 5 * NL * stride, stride, p.z.c1);
}
BN_FUNC G2P ks_load_point(const int32_t* ws, size_t stride) {
  return {{load_fp(ws, stride), load_fp(ws + NL * stride, stride)},
          {load_fp(ws + 2 * NL * stride, stride), load_fp(ws + 3 * NL * stride, stride)},
          {load_fp(ws + 4 * NL * stride, stride), load_fp(ws + 5 * NL * stride, stride)}};
}

// tile: the word's 32 keys, limb-major [KS_AFF_LIMBS][32]
BN_FUNC G2P ks_word_sum(uint32_t m, const int32_t* tile) {
  BN_CTX;
  G2P acc = proj_identity<Fp2>();
#pragma unroll 1
  while (m) {
    const uint32_t j = ks_ctz(m);
    m &= m - 1;
    acc = proj_add_mixed(acc, ks_load_aff(tile + j, 32));
  }
  return acc;
}
// run k of group g in a pass over `cnt` partials per group: items (KS_RUN k + i) G + g, i < min(KS_RUN, cnt - KS_RUN k)
BN_FUNC G2P ks_group_run(const int32_t* in, size_t in_stride, size_t G, size_t g, uint32_t k, uint32_t cnt) {
  BN_CTX;
  const uint32_t first = KS_RUN * k, len = cnt - first < KS_RUN ? cnt - first : KS_RUN;
  G2P acc = proj_identity<Fp2>();
#pragma unroll 1
  for (uint32_t i = 0; i < len; ++i) acc = proj_add(acc, ks_load_point(in + (size_t)(first + i) * G + g, in_stride));
  return acc;
}
BN_FUNC G2P ks_finish(const G2P& u, const G2P& total, bool flip, bool ok) {
  BN_CTX;
  G2P r = u;
  if (flip) r = proj_add(total, proj_neg(u));
  return proj_select(ok, r, proj_identity<Fp2>());
}

}  // namespace bn
