// keyset_committee.h -- what ONE lane does in the calls over COMMITTEES of a registered key set (k_keyset_committee.hip,
// host_keyset_committee.hip).  A committee is a list of key indices kept on the handle (members, and per committee
// {first member, size, word base}: KcCom); a group names a committee and brings a row as wide as it, bit j (LSB-first) = member
// j signed.  Everything keyset.h does per 32-key word of the REGISTRY is done here per 32-member word of a COMMITTEE, through
// one indirection, and with the functions of keyset.h themselves:
//   kc_word_bits    registration of a table: the bad / skip / valid bits of a committee word, bit j = that bit of key
//                   members[base + j] in the handle's words (0 past the committee's end)
//   kc_count        ks_count over the committee's words: the flip threshold is the COMMITTEE's size
//   kc_tile_limb    the staging gather: element (limb, j) of the [KS_AFF_LIMBS][32] tile ks_word_sum reads, the affine row of
//                   member j of the word, zeros past the committee's end
//   kc_lane_sum     kw_lane_sum (keyset_weight.h) over a committee's words, the table row found through the member list
// The sums themselves are ks_word_mask / ks_word_sum / ks_finish of keyset.h, unchanged.  keyset_committee_plan.h (included here)
// is the plain C++ of the host side.  tests/hostsim/keyset_committee_host.cpp compiles both for the host with -DBN_CHECK.  The
// lane functions are not a CPU fallback: nothing in the product's host path calls them.
#pragma once
#include "keyset.h"
#include "keyset_weight.h"
#include "keyset_committee_plan.h"

namespace bn {

constexpr uint32_t KC_LANES = 64;                // lanes of one item of the word kernel: one wave
static_assert(KC_LANES == KC_ITEM_GROUPS && KS_RUN == KC_RUN, "keyset_committee_plan.h");

BN_INL uint32_t kc_bit(const uint32_t* words, uint32_t key) { return (words[key >> 5] >> (key & 31)) & 1u; }
// mem: the word's members (left = how many of its 32 positions name one, 1 .. 32)
struct KcBits { uint32_t bad, skip, valid; };
BN_INL KcBits kc_word_bits(const uint32_t* mem, uint32_t left, const uint32_t* bad, const uint32_t* skip, const uint32_t* vwords) {
  KcBits o = {0, 0, 0};
#pragma unroll
  for (uint32_t j = 0; j < 32; ++j)
    if (j < left) {
      const uint32_t key = mem[j];
      o.bad |= kc_bit(bad, key) << j; o.skip |= kc_bit(skip, key) << j; o.valid |= kc_bit(vwords, key) << j;
    }
  return o;
}
// the positions of word w of a committee of `size` members that name one
BN_INL uint32_t kc_left(uint32_t size, uint32_t w) { return size - 32 * w < 32 ? size - 32 * w : 32; }
// cbad: the committee's bad words (at its word base).  noflip: the totals of a table are summed directly
BN_INL KsCount kc_count(const uint8_t* row, uint32_t size, const uint32_t* cbad, bool noflip) {
  KsCount c = ks_count(row, size, cbad);
  c.flip = c.flip & !noflip;
  return c;
}
// mem: the word's members (staged), t = 32 limb + j
BN_INL int32_t kc_tile_limb(const int32_t* aff, uint32_t n_keys, const uint32_t* mem, uint32_t left, uint32_t t) {
  const uint32_t j = t & 31;
  return j < left ? aff[(size_t)(t >> 5) * n_keys + mem[j]] : 0;
}
// members: the committee's (at its first member); cvalid: its validity words (at its word base)
BN_INL KwAcc kc_lane_sum(const uint8_t* row, uint32_t size, uint32_t lane, const uint32_t* cvalid, const uint32_t* members, const uint64_t* tab,
                         uint32_t n_cols) {
  const uint32_t W = ks_words(size), rb = ks_row_bytes(size);
  KwAcc a;
#pragma unroll
  for (uint32_t q = 0; q < KW_COLS; ++q) a.v[q] = 0;
#pragma unroll 1
  for (uint32_t w = lane; w < W; w += KW_WAVE) {
    uint32_t m = ks_row_word(row, rb, w) & ks_tail_mask(size, w) & cvalid[w];
#pragma unroll 1
    while (m) {
      const uint32_t j = ks_ctz(m);
      m &= m - 1;
      kw_add_key(a, tab, n_cols, members[32 * w + j]);
    }
  }
  return a;
}

}  // namespace bn
