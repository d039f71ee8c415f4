// k_keyset.hip -- sums over a registered key set selected by bitmaps (keyset.h has the lane functions and the layout):
//   k_ks_register    one lane per key, once per key set: affine rows, the bad / skip words (by ballot), KeyValidate bytes; with a
//                    mask (the bits of the proofs of possession) a key whose bit is 0 is BAD as one that does not decode, and
//                    the lane stores an undecodable encoding over ITS key in the staged copy it read, so that the total (a
//                    segmented sum over the staged encodings, which loads a bad key as the identity) leaves the key out
//   k_ks_count       one lane per group: flip and ok of its row
//   k_ks_word_sum    the hot kernel: grid (ceil(G / 256), W), a workgroup is ONE 32-key word across 256 consecutive groups.  The
//                    word's keys are staged into LDS once (36 x 32 limbs, 4.6 KB, [limb][32]: for a fixed limb the 32 keys sit
//                    in 32 banks, lanes that want the same key get a broadcast); a lane walks the set bits of its mask with
//                    mixed additions and stores its partial word-major
//   k_ks_group_sum   one lane per (group, run of 16 partials), pass after pass until one partial per group is left; the last
//                    pass applies the complement and writes the group's column of the sums the verify pipeline encodes
// Groups are uniform, so there are no run descriptors: nothing but the rows, flip and ok bytes is read to find a lane's work.
// Plain vector stores, no atomics; nothing synchronises between the passes.
#include "keyset.h"
#include "kernels.h"
using namespace bn;

BN_KERNEL k_ks_register(uint8_t* pks, uint32_t n_keys, const uint8_t* sub_ok, const uint8_t* mask, int32_t* aff, uint32_t* bad, uint32_t* skip, uint8_t* valid) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool b = false, s = false;
  if (i < n_keys) {
    const KsKey k = ks_register(pks + 128 * (size_t)i);
    const bool pass = ks_mask_bit(mask, i);
    b = k.bad | !pass; s = k.skip | !pass;
    if (!pass) ks_blank_enc(pks + 128 * (size_t)i);
    ks_store_aff(aff + i, n_keys, k.p);
    valid[i] = (sub_ok[i] && !s) ? 1 : 0;
  }
  // a wave's 64 keys are two words; lanes past n_keys vote 0
  const unsigned long long mb = __ballot(b), ms = __ballot(s);
  const uint32_t lane = threadIdx.x & 63, w = (i - lane) / 32 + lane;
  if (lane < 2 && w < ks_words(n_keys)) { bad[w] = (uint32_t)(mb >> (32 * lane)); skip[w] = (uint32_t)(ms >> (32 * lane)); }
}

BN_KERNEL k_ks_count(const uint8_t* sel, size_t G, uint32_t n_keys, const uint32_t* bad, uint8_t* flip, uint8_t* ok) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const KsCount c = ks_count(sel + g * ks_row_bytes(n_keys), n_keys, bad);
  flip[g] = c.flip ? 1 : 0;
  ok[g] = c.ok ? 1 : 0;
}

BN_KERNEL k_ks_word_sum(const int32_t* aff, uint32_t n_keys, const uint32_t* skip, const uint8_t* sel, const uint8_t* flip, size_t G,
                        int32_t* out, size_t out_stride) {
  __shared__ int32_t tile[KS_AFF_LIMBS * 32];
  const uint32_t w = blockIdx.y;
  for (uint32_t t = threadIdx.x; t < KS_AFF_LIMBS * 32; t += blockDim.x) {
    const uint32_t key = 32 * w + (t & 31);
    tile[t] = key < n_keys ? aff[(size_t)(t >> 5) * n_keys + key] : 0;
  }
  __syncthreads();
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const uint32_t rb = ks_row_bytes(n_keys);
  const uint32_t m = ks_word_mask(ks_row_word(sel + g * rb, rb, w), flip[g] != 0, skip[w], ks_tail_mask(n_keys, w));
  ks_store_point(out + (size_t)w * G + g, out_stride, ks_word_sum(m, tile));
}

// cnt partials per group in (stride in_stride), ceil(cnt / KS_RUN) per group out (stride out_stride).  last (one run per group):
// the complement against `total` and the flags; out / ok_out are then the groups' columns of the call's sums.
BN_KERNEL k_ks_group_sum(const int32_t* in, size_t in_stride, uint32_t cnt, size_t G, const uint8_t* flip, const uint8_t* ok, const int32_t* total,
                         int last, int32_t* out, size_t out_stride, uint8_t* ok_out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t runs = (cnt + KS_RUN - 1) / KS_RUN;
  if (i >= (size_t)runs * G) return;
  const uint32_t k = (uint32_t)(i / G);
  const size_t g = i - (size_t)k * G;
  G2P acc = ks_group_run(in, in_stride, G, g, k, cnt);
  if (last) {
    acc = ks_finish(acc, ks_load_point(total, 1), flip[g] != 0, ok[g] != 0);
    ok_out[g] = ok[g];
  }
  ks_store_point(out + i, out_stride, acc);
}
