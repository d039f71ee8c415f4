// k_keyset_committee.hip -- sums and stake weights over COMMITTEES of a registered key set (keyset_committee.h has the lane
// functions, keyset_committee_plan.h the plan; host_keyset_committee.hip):
//   k_kc_words       once per table, one lane per committee word: its bad / skip / valid words out of the handle's
//   k_kc_count       one lane per sorted group: flip (against the COMMITTEE's size) and ok of its row
//   k_kc_word_sum    the hot kernel: a workgroup of ONE wave is one ITEM of the plan, one 32-member word of one committee across
//                    up to 64 consecutive sorted groups of that committee.  The word's member indices go to LDS, then the
//                    members' affine rows are gathered through them into the [limb][32] tile of k_ks_word_sum (4.6 KB); lane l
//                    takes sorted group first + l, walks the set bits of its mask with mixed additions (ks_word_sum, keyset.h)
//                    and stores its partial GROUP-major: partial pbase[group] + w of the launch
//   k_kc_finish      one lane per sorted group, behind the segmented reduction of the partials (k_g2_seg_sum): the complement
//                    against the committee's total and the flags, stored into the CALLER's column order[i] of the sums the verify
//                    pipeline encodes
//   k_kc_weight      one wave per group, the layout and reduction of k_ks_weight, the table row found through the member list
// Plain vector stores, no atomics; no lane reads what another lane of the same launch wrote.
#include "keyset_committee.h"
#include "kernels.h"
using namespace bn;

BN_KERNEL k_kc_words(const uint32_t* members, const uint4* coms, const uint32_t* wcom, size_t n_words, const uint32_t* bad, const uint32_t* skip,
                     const uint32_t* vwords, uint32_t* cbad, uint32_t* cskip, uint32_t* cvalid) {
  const size_t cw = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (cw >= n_words) return;
  const uint4 k = coms[wcom[cw]];                        // off, size, wbase
  const uint32_t w = (uint32_t)cw - k.z;
  const KcBits b = kc_word_bits(members + k.x + 32 * w, kc_left(k.y, w), bad, skip, vwords);
  cbad[cw] = b.bad; cskip[cw] = b.skip; cvalid[cw] = b.valid;
}

// sorted groups lo .. lo + m of the call
BN_KERNEL k_kc_count(const uint8_t* sel, const uint64_t* srow, const uint32_t* scom, const uint4* coms, const uint32_t* cbad, size_t lo, size_t m, int noflip,
                     uint8_t* flip, uint8_t* ok) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m) return;
  const size_t i = lo + t;
  const uint4 k = coms[scom[i]];
  const KsCount c = kc_count(sel + srow[i], k.y, cbad + k.z, noflip != 0);
  flip[i] = c.flip ? 1 : 0;
  ok[i] = c.ok ? 1 : 0;
}

// items: the launch's; out: its partials (stride out_stride = their number); the per-group arrays are the call's
BN_KERNEL k_kc_word_sum(const int32_t* aff, uint32_t n_keys, const uint32_t* members, const uint4* coms, const uint32_t* cskip, const uint4* items, const uint8_t* sel,
              const uint64_t* srow, const uint32_t* scom, const uint32_t* spbase, const uint8_t* flip, int32_t* out, size_t out_stride) {
  __shared__ uint32_t mem[32];
  __shared__ int32_t tile[KS_AFF_LIMBS * 32];
  const uint4 it = items[blockIdx.x];                    // cword, mbase, first, count
  const uint4 k = coms[scom[it.z]];
  const uint32_t w = it.x - k.z, left = kc_left(k.y, w);
  if (threadIdx.x < 32) mem[threadIdx.x] = threadIdx.x < left ? members[it.y + threadIdx.x] : 0;
  __syncthreads();
  for (uint32_t t = threadIdx.x; t < KS_AFF_LIMBS * 32; t += KC_LANES) tile[t] = kc_tile_limb(aff, n_keys, mem, left, t);
  __syncthreads();
  if (threadIdx.x >= it.w) return;
  const size_t i = (size_t)it.z + threadIdx.x;
  const uint32_t m = ks_word_mask(ks_row_word(sel + srow[i], ks_row_bytes(k.y), w), flip[i] != 0, cskip[it.x], ks_tail_mask(k.y, w));
  ks_store_point(out + spbase[i] + w, out_stride, ks_word_sum(m, tile));
}

// u: the call's reduced sums by sorted position (stride u_stride); totals: the committees' (stride n_com)
BN_KERNEL k_kc_finish(const int32_t* u, size_t u_stride, size_t G, const uint32_t* scom, const uint32_t* order, const int32_t* totals, size_t n_com,
                      const uint8_t* flip, const uint8_t* ok, int32_t* out, size_t out_stride, uint8_t* ok_out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= G) return;
  const size_t g = order[i];
  const G2P r = ks_finish(ks_load_point(u + i, u_stride), ks_load_point(totals + scom[i], n_com), flip[i] != 0, ok[i] != 0);
  ks_store_point(out + g, out_stride, r);
  ok_out[g] = ok[i];
}

// Launch of m groups = groups g_lo .. g_lo + m of the call, in the caller's order.  grow / gcom: the groups' row offsets and
// committees; out[g n_cols + q].
__global__ void __launch_bounds__(256) k_kc_weight(const uint8_t* rows, const uint64_t* grow, const uint32_t* gcom, const uint4* coms, const uint32_t* members,
                                                  const uint32_t* cvalid, const uint64_t* tab, uint32_t n_cols, size_t g_lo, size_t m, uint64_t* out) {
  const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (wave >= m) return;                                 // the whole wave
  const uint32_t lane = threadIdx.x & 63;
  const size_t g = g_lo + wave;
  const uint4 k = coms[gcom[g]];
  KwAcc a = kc_lane_sum(rows + grow[g], k.y, lane, cvalid + k.z, members + k.x, tab, n_cols);
#pragma unroll
  for (uint32_t d = KW_WAVE / 2; d; d >>= 1) {
#pragma unroll
    for (uint32_t q = 0; q < KW_COLS; ++q)
      if (q < n_cols) {                                  // uniform: every lane of the wave takes part in the shuffle
        const uint32_t lo = (uint32_t)__shfl_down((int)kw_lo(a.v[q]), d), hi = (uint32_t)__shfl_down((int)kw_hi(a.v[q]), d);
        a.v[q] += kw_join(lo, hi);                       // lanes >= 64 - d add their own value: never read by lane 0's chain
      }
  }
  if (lane == 0) {
#pragma unroll
    for (uint32_t q = 0; q < KW_COLS; ++q)
      if (q < n_cols) out[g * n_cols + q] = a.v[q];
  }
}
