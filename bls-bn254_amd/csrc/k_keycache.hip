// k_keycache.hip -- the per-context store of prepared keys (key_cache.h): a key whose 128 bytes an earlier call on the context
// prepared is not prepared again.  Behind the batch's de-duplication (k_keyprep.hip: keys[j] = representative tuple of distinct key
// j, *batch_cnt of them) a call runs begin -> clear -> lookup, then the per-key preparation (k_g2_prepare / _quad, k_g2_expand)
// over the MISS list only, dense as without a store and bounded by the device-side miss count, and scatter copies the misses'
// tables and validity bytes into their places.  Tuples keep their batch key ids for the key-sorted order; k_kd_cache_map
// gives every tuple its key's store index, which is what the table-only Miller kernels then take as the key id.
// No field arithmetic in here: these kernels move indices and bytes.
#include "kernels.h"
#include "key_cache.h"
using namespace bn;

__global__ void k_kd_cache_begin(const uint32_t* batch_cnt, uint32_t bound, uint32_t C, uint32_t R, uint32_t* st, unsigned long long* stats) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  kc_begin(st, stats, *batch_cnt, bound, C, R);
}
__global__ void k_kd_cache_clear(const uint32_t* st, uint32_t* slots, uint32_t m) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) kc_clear(st, slots, i);
}
// slot_of[j] for the batch's distinct keys j < st[KC_BATCH]; a miss appends (representative tuple, store index) to the miss list
__global__ void k_kd_cache_lookup(const uint8_t* pks, const uint32_t* keys, uint32_t* st, uint32_t* slots, uint32_t mask, uint32_t seed, uint8_t* store_keys,
                                  uint32_t* slot_of, uint32_t* miss_rep, uint32_t* miss_slot) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= st[KC_BATCH]) return;
  const uint32_t rep = keys[j];
  const KcFound f = kc_lookup(pks + 128 * (size_t)rep, seed, slots, mask, store_keys, st[KC_COUNT], &st[KC_MISS]);
  slot_of[j] = f.slot;
  if (f.miss != KC_EMPTY) { miss_rep[f.miss] = rep; miss_slot[f.miss] = f.slot; }
}
// dense: the misses' pair tables in miss-list order (key_words 16-byte words each), dense_ok: their validity bytes.  A fixed
// grid strides over st[KC_MISS] x key_words words: with no miss the launch leaves at once.  One lane closes the call (kc_end).
__global__ void __launch_bounds__(256) k_kd_cache_scatter(const int4* dense, const uint8_t* dense_ok, const uint32_t* miss_slot, uint32_t key_words, uint32_t* st,
                                                          unsigned long long* stats, int4* table, uint8_t* valid) {
  const uint32_t misses = st[KC_MISS];
  const size_t total = (size_t)misses * key_words, step = (size_t)gridDim.x * blockDim.x;
  for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += step) {
    const uint32_t m = (uint32_t)(x / key_words), w = (uint32_t)(x - (size_t)m * key_words);
    table[(size_t)miss_slot[m] * key_words + w] = dense[x];
    if (w == 0) valid[miss_slot[m]] = dense_ok[m];
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == blockDim.x - 1) kc_end(st, stats);      // st[KC_MISS] stays as the others read it
}
// out[i] = slot_of[ids[i]]: tuples (or chunks of tuples) from batch key ids to store indices
__global__ void k_kd_cache_map(const uint32_t* ids, uint32_t n, const uint32_t* slot_of, uint32_t* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = slot_of[ids[i]];
}
// ok[j] = valid[slot_of[j]]: the validity bytes in batch key order, for the kernels that index them by batch key id
__global__ void k_kd_cache_ok(const uint32_t* slot_of, uint32_t u, const uint8_t* valid, uint8_t* ok) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < u) ok[j] = valid[slot_of[j]];
}
