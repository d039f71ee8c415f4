// k_msg_distinct.hip -- the distinct-message rule of the aggregate verify over groups on the device: one lane per pair, the lane
// functions of msg_distinct.h behind their tuple index.  k_md_keys leaves the canonical (x, y) of every hash point, k_md_insert
// puts (group, x, y) into the call's table and marks the groups where a key is met twice (host_msg_distinct.hip clears the table
// and dup[] on the stream before them).  Own translation unit, field functions force-inlined (the hash unit's policy).
#include "msg_distinct.h"
using namespace bn;

__global__ void __launch_bounds__(256) k_md_keys(const int32_t* pts, size_t stride, uint32_t n, int form, int32_t* key) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  md_key(pts + i, stride, form, key + i, n);
}
__global__ void __launch_bounds__(256) k_md_insert(uint32_t n, const uint32_t* goff, uint32_t G, const int32_t* key, uint32_t* slots, uint32_t mask, uint32_t seed,
                                                   uint8_t* dup) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  md_insert(i, n, goff, G, key, slots, mask, seed, dup);
}
