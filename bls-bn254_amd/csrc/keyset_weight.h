// keyset_weight.h -- what ONE lane does in the stake weights over a REGISTERED key set selected by bitmaps (k_keyset_weight.hip,
// host_keyset_weight.hip).  A key set may carry a table of n_cols <= KW_COLS stake columns, unsigned 64-bit, whose column sums
// over all keys fit 64 bits (checked by the host, keyset_weight_plan.h), so that no sum here can overflow.
// The table is on the device KEY-major (tab[i n_cols + q], transposed by the host, kw_key_major): the columns of one key are
// neighbours, so a selected key costs one cache line whatever n_cols.  The EFFECTIVE weight of a key without the KeyValidate bit
// is 0: the lane ANDs every word of the row with the key set's validity word (vwords, packed once at registration) before it
// walks the bits, so such a key is never added, whatever the table holds for it.
//   kw_lane_sum     one lane of the WAVE that weighs a row, lane l owning the 32-key words l, l + 64, ...: the lane walks the
//                   set bits of its words that name a valid key and adds the keys' columns into KW_COLS accumulators.  The
//                   loop over the columns has a constant trip count and is fully unrolled, so the accumulators are registers:
//                   nothing indexes them
//   kw_lo / kw_hi / kw_join   the wave reduction hands a 64-bit value from lane to lane as its two 32-bit halves
// Rows are byte arrays whose length is in general no multiple of 4: they are read as ks_count reads them (ks_row_word).  Bits
// past the last key are masked (ks_tail_mask), though the host refuses a row that sets one.
// keyset_weight_plan.h (included here) is the plain C++ of the host side.  tests/hostsim/keyset_weight_host.cpp compiles both for
// the host, runs a wave as 64 lane states and carries the halves between them itself.  The lane functions are not a CPU
// fallback: nothing in the product's host path calls them.
#pragma once
#include "keyset.h"
#include "keyset_weight_plan.h"

namespace bn {

constexpr uint32_t KW_WAVE = 64;                 // lanes that share a group; the stride of a lane's words
constexpr uint32_t KW_COLS = 8;                  // BLSBN254_KS_MAX_COLS
static_assert(KW_COLS == KW_MAX_COLS && KW_WAVE == KW_WAVE_LANES, "keyset_weight_plan.h");

struct KwAcc { uint64_t v[KW_COLS]; };           // indexed by unrolled constants only

BN_INL void kw_add_key(KwAcc& a, const uint64_t* tab, uint32_t n_cols, uint32_t key) {
  const uint64_t* e = tab + (size_t)key * n_cols;
#pragma unroll
  for (uint32_t q = 0; q < KW_COLS; ++q)
    if (q < n_cols) a.v[q] += e[q];
}
// vwords: the key set's KeyValidate bits, a word per 32 keys (bits past the last key 0)
BN_INL KwAcc kw_lane_sum(const uint8_t* row, uint32_t n_keys, uint32_t lane, const uint32_t* vwords, const uint64_t* tab, uint32_t n_cols) {
  const uint32_t W = ks_words(n_keys), rb = ks_row_bytes(n_keys);
  KwAcc a;
#pragma unroll
  for (uint32_t q = 0; q < KW_COLS; ++q) a.v[q] = 0;
#pragma unroll 1
  for (uint32_t w = lane; w < W; w += KW_WAVE) {
    uint32_t m = ks_row_word(row, rb, w) & ks_tail_mask(n_keys, w) & vwords[w];
#pragma unroll 1
    while (m) {
      const uint32_t j = ks_ctz(m);
      m &= m - 1;
      kw_add_key(a, tab, n_cols, 32 * w + j);
    }
  }
  return a;
}
BN_INL uint32_t kw_lo(uint64_t v) { return (uint32_t)v; }
BN_INL uint32_t kw_hi(uint64_t v) { return (uint32_t)(v >> 32); }
BN_INL uint64_t kw_join(uint32_t lo, uint32_t hi) { return (uint64_t)hi << 32 | lo; }

}  // namespace bn
