// k_keyset_weight.hip -- stake weights over a registered key set selected by bitmaps (keyset_weight.h has the lane functions;
// host_keyset_weight.hip):
//   k_ks_weight        the hot kernel: ONE WAVE per group, four groups per workgroup (the layout of k_km_select), lane l owning
//                      the 32-key words l, l + 64, ... of the row.  The lane walks the set bits of its words that name a key
//                      with the KeyValidate bit (the effective weight of any other key is 0) and adds the keys' columns into
//                      eight 64-bit accumulators (a fully unrolled loop over the columns: registers, no scratch);
//                      six rounds of cross-lane shuffles of the two 32-bit halves fold the wave's accumulators into lane 0, which
//                      stores the group's n_cols sums.  The table is read from global memory: at most 4 MB and usually 64 KB, it
//                      stays in L2 (DESIGN.md 6k has the measurement behind that choice)
// No lane reads what another lane of any launch wrote: plain vector stores, no atomics.  Integer addition makes the result
// independent of the order of the lanes and of where a launch ended.  Launches end on group boundaries.
#include "keyset_weight.h"
#include "kernels.h"
using namespace bn;

// Launch of m groups = groups g_lo .. g_lo + m of the call.  rows: the call's rows of ceil(n_keys / 8) bytes; vwords: the key set's
// KeyValidate bits by words; tab: its table, key-major; out: the call's n_groups x n_cols sums, out[g n_cols + q].
__global__ void __launch_bounds__(256) k_ks_weight(const uint8_t* rows, const uint32_t* vwords, const uint64_t* tab, uint32_t n_keys, uint32_t n_cols, size_t g_lo,
                                                  size_t m, uint64_t* out) {
  const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (wave >= m) return;                                 // the whole wave
  const uint32_t lane = threadIdx.x & 63;
  const size_t g = g_lo + wave;
  KwAcc a = kw_lane_sum(rows + g * ks_row_bytes(n_keys), n_keys, lane, vwords, tab, n_cols);
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
