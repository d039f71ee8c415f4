// keyset_host.cpp -- proj_add_mixed (csrc/curve.h) and the lane functions of csrc/keyset.h (sums over a registered key set selected
// by bitmaps) compiled for the host with -DBN_CHECK (every field operation asserts the lazy-limb interval discipline), for
// tests/test_keyset_host.py: registration, flip / ok, the per-word masks, the word sums out of a staged tile, the reduction
// passes over word-major partials and the complement, run lane by lane as the kernels of k_keyset.hip index them.  TEST TOOL ONLY.
#include "../../bls-bn254_amd/csrc/keyset.h"
#include <cstring>
#include <vector>

using namespace bn;

extern "C" {

// P = identity (p_identity) or 2 A (a projective point with Z != 1); out_mixed = P + Q by proj_add_mixed, out_full = P + Q by
// proj_add on proj_from_affine(Q).  Returns 0 when A or Q does not decode.
int hs_ks_add_mixed(const uint8_t a[128], int p_identity, const uint8_t q[128], uint8_t out_mixed[128], uint8_t out_full[128]) {
  bool oka, okq;
  const G2A A = g2_decode(a, oka), Q = g2_decode(q, okq);
  if (!oka || !okq || Q.inf) return 0;
  const G2P P = p_identity ? proj_identity<Fp2>() : proj_dbl(proj_from_affine(A));
  g2_encode(out_mixed, g2_to_affine(proj_add_mixed(P, Q)));
  g2_encode(out_full, g2_to_affine(proj_add(P, proj_from_affine(Q))));
  return 1;
}

// The whole pipeline over one launch of G rows: registration (k_ks_register), the total, k_ks_count, k_ks_word_sum with its tile,
// the k_ks_group_sum passes.  bad / skip: W words each; flip / ok: G bytes; masks: W x G words, word-major; out: G x 128 bytes.
// Returns the number of reduction passes.
int hs_ks_run(const uint8_t* pks, uint32_t n_keys, const uint8_t* sel, uint32_t G, uint32_t* bad, uint32_t* skip, uint8_t* flip, uint8_t* ok,
              uint32_t* masks, uint8_t* out) {
  const uint32_t W = ks_words(n_keys), rb = ks_row_bytes(n_keys);
  std::vector<int32_t> aff((size_t)KS_AFF_LIMBS * n_keys), total(6 * NL);
  G2P T = proj_identity<Fp2>();
  for (uint32_t w = 0; w < W; ++w) bad[w] = skip[w] = 0;
  for (uint32_t i = 0; i < n_keys; ++i) {
    const KsKey k = ks_register(pks + 128 * (size_t)i);
    ks_store_aff(aff.data() + i, n_keys, k.p);
    if (k.bad) bad[i / 32] |= 1u << (i % 32);
    if (k.skip) skip[i / 32] |= 1u << (i % 32);
    if (!k.skip) T = proj_add(T, proj_from_affine(k.p));
  }
  ks_store_point(total.data(), 1, T);
  for (uint32_t g = 0; g < G; ++g) {
    const KsCount c = ks_count(sel + (size_t)g * rb, n_keys, bad);
    flip[g] = c.flip; ok[g] = c.ok;
  }
  std::vector<int32_t> part[2];
  size_t stride = (size_t)W * G;
  part[0].assign(6 * NL * stride, 0);
  for (uint32_t w = 0; w < W; ++w) {
    int32_t tile[KS_AFF_LIMBS * 32];
    for (uint32_t t = 0; t < KS_AFF_LIMBS * 32; ++t) {
      const uint32_t key = 32 * w + (t & 31);
      tile[t] = key < n_keys ? aff[(size_t)(t >> 5) * n_keys + key] : 0;
    }
    for (uint32_t g = 0; g < G; ++g) {
      const uint32_t m = ks_word_mask(ks_row_word(sel + (size_t)g * rb, rb, w), flip[g] != 0, skip[w], ks_tail_mask(n_keys, w));
      masks[(size_t)w * G + g] = m;
      ks_store_point(part[0].data() + (size_t)w * G + g, stride, ks_word_sum(m, tile));
    }
  }
  int passes = 0, src = 0;
  for (uint32_t cnt = W;; ++passes) {
    const uint32_t runs = (cnt + KS_RUN - 1) / KS_RUN;
    const bool last = runs == 1;
    const size_t ostride = (size_t)runs * G;
    part[src ^ 1].assign(6 * NL * ostride, 0);
    for (size_t i = 0; i < ostride; ++i) {
      const uint32_t k = (uint32_t)(i / G);
      const size_t g = i - (size_t)k * G;
      G2P acc = ks_group_run(part[src].data(), stride, G, g, k, cnt);
      if (last) acc = ks_finish(acc, ks_load_point(total.data(), 1), flip[g] != 0, ok[g] != 0);
      ks_store_point(part[src ^ 1].data() + i, ostride, acc);
    }
    src ^= 1; stride = ostride; cnt = runs;
    if (last) { ++passes; break; }
  }
  for (uint32_t g = 0; g < G; ++g) g2_encode(out + 128 * (size_t)g, g2_to_affine(ks_load_point(part[src].data() + g, stride)));
  return passes;
}

}  // extern "C"
