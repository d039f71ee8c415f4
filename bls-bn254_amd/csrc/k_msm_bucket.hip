// k_msm_bucket.hip -- multi-scalar multiplication sum_i [k_i] P_i by the bucket method (msm.h), G1 and G2 from one source.
// Phases (one launch each, host_msm.hip):
//   k_msm_g{1,2}_prep     lane per point: decode + on-curve + scalar < r (status), affine rows, signed digits -> bucket entries
//   k_kd_msm_hist         per-window counting of the entries by bucket (LDS histogram, one global atomic per bucket and tile)
//   k_scan_excl           (k_keyprep.hip) bucket starts
//   k_kd_msm_scatter      entries in bucket order (LDS ranks, one global atomic per bucket and tile)
//   k_msm_g{1,2}_bucket   levels of chunk sums, lane per chunk of <= 32 inputs of one bucket
//   k_msm_g{1,2}_reduce   lane per (window, segment): sum_j j S_j by running sums
//   k_msm_g{1,2}_final    one workgroup: segments per window in LDS, Horner over the windows, affine bytes
#include "msm.h"
#include "fr29.h"
#include "kernels.h"
using namespace bn;

namespace {
constexpr int MSM_EPL = 8;                       // entries per lane of the sort kernels: a tile of 2048 entries per workgroup
constexpr uint32_t MSM_TILE = 256 * MSM_EPL;
constexpr uint32_t MSM_LDS_KEYS = 8192;          // buckets counted per pass in LDS (32 KiB); 2^(c-1) > 8192 takes several passes

// the tile's keys of window blockIdx.y (entries w * S + [tile, tile + MSM_TILE) that exist; MSM_NO_KEY beyond S)
__device__ inline void load_tile_keys(const uint32_t* key, size_t S, uint32_t k[MSM_EPL], size_t idx[MSM_EPL]) {
  const size_t t0 = (size_t)blockIdx.x * MSM_TILE;
  for (int e = 0; e < MSM_EPL; ++e) {
    const size_t i = t0 + (size_t)e * 256 + threadIdx.x;
    idx[e] = (size_t)blockIdx.y * S + i;
    k[e] = i < S ? key[idx[e]] : MSM_NO_KEY;
  }
}

__device__ inline void msm_encode(uint8_t* out, const G1P& p) { g1_encode(out, g1_to_affine(p)); }
__device__ inline void msm_encode(uint8_t* out, const G2P& p) { g2_encode(out, g2_to_affine(p)); }

// one workgroup of 256: window w = W-1 .. 0: acc = 2^c acc + sum_g seg[w][g] (the G <= 256 segments summed in LDS); bytes.
// stats[0] = bucket entries, stats[1] = level-0 chunks (sum over buckets of ceil(h / L)).
template <class F> __device__ void msm_final(const int32_t* seg, uint32_t W, uint32_t G, int c, const uint32_t* hist, uint32_t u,
                                             uint8_t* out, uint32_t* stats) {
  constexpr int K = FLimbs<F>::n;
  __shared__ int32_t lds[3 * K * 256];
  __shared__ uint32_t cnt[2];
  const unsigned tid = threadIdx.x;
  if (tid == 0) { cnt[0] = 0; cnt[1] = 0; }
  __syncthreads();
  uint32_t ent = 0, chk = 0;
  for (uint32_t b = tid; b < u; b += 256) { const uint32_t h = hist[b]; ent += h; chk += msm_level_inputs(h, 1); }
  atomicAdd(&cnt[0], ent); atomicAdd(&cnt[1], chk);
  Proj<F> acc = proj_identity<F>();
  const size_t seg_st = (size_t)W * G;
  for (uint32_t w = W; w-- > 0;) {
    Proj<F> s = proj_identity<F>();
    if (tid < G) s = msm_load_p<F>(seg + (size_t)w * G + tid, seg_st);
    for (unsigned h = 128; h > 0; h >>= 1) {
      if (tid >= h && tid < 2 * h) msm_store_p(lds + tid, 256, s);
      __syncthreads();
      if (tid < h) s = proj_add(s, msm_load_p<F>(lds + tid + h, 256));
      __syncthreads();
    }
    if (tid == 0) {
#pragma unroll 1
      for (int d = 0; d < c; ++d) acc = proj_dbl(acc);
      acc = proj_add(acc, s);
    }
  }
  __syncthreads();
  if (tid == 0) {
    msm_encode(out, acc);
    stats[0] = cnt[0]; stats[1] = cnt[1];
  }
}
}  // namespace

// ---------------------------------------------------------------- recoding
// G1: rows i = P_i and n + i = phi(P_i) = (beta x, y) (2n rows, x then y, 9 limbs each); entries of half h at w * 2n + h n + i
BN_KERNEL k_msm_g1_prep(const uint8_t* g1, const uint8_t* scalars, size_t n, int c, int W, int32_t* pts, uint32_t* key, uint32_t* val, uint8_t* status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bool okd, oks;
  G1A p = g1_decode(g1 + 64 * i, okd);
  const bool okp = okd & g1_on_curve(p);
  (void)fr_from_be(scalars + 32 * i, oks);
  uint32_t k[8];
  msm_scalar_words(scalars + 32 * i, k);
  const bool live = okp & oks & !p.inf;
  const size_t rows = 2 * n;
  msm_store(pts + i, rows, p.x); msm_store(pts + NL * rows + i, rows, p.y);
  msm_store(pts + n + i, rows, fp_mul(p.x, fp_const(bnc::GLV_BETA))); msm_store(pts + NL * rows + n + i, rows, p.y);
  const GlvSplit g = glv_split(k);
  msm_recode_store<4>(g.k1, c, W, g.neg1, live, (uint32_t)i, key + i, val + i, rows);
  msm_recode_store<4>(g.k2, c, W, g.neg2, live, (uint32_t)(n + i), key + n + i, val + n + i, rows);
  status[i] = (uint8_t)((okp ? 1 : 0) | (oks ? 2 : 0));
}
// G2: rows i = P_i (n rows, x then y, 18 limbs each), the full 254-bit scalar; entries at w * n + i
BN_KERNEL k_msm_g2_prep(const uint8_t* g2, const uint8_t* scalars, size_t n, int c, int W, int32_t* pts, uint32_t* key, uint32_t* val, uint8_t* status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bool okd, oks;
  G2A p = g2_decode(g2 + 128 * i, okd);
  const bool okp = okd & g2_on_curve(p);
  (void)fr_from_be(scalars + 32 * i, oks);
  uint32_t k[8];
  msm_scalar_words(scalars + 32 * i, k);
  const bool live = okp & oks & !p.inf;
  msm_store(pts + i, n, p.x); msm_store(pts + 2 * NL * n + i, n, p.y);
  msm_recode_store<8>(k, c, W, false, live, (uint32_t)i, key + i, val + i, n);
  status[i] = (uint8_t)((okp ? 1 : 0) | (oks ? 2 : 0));
}

// ---------------------------------------------------------------- counting sort by (window, bucket)
// grid (ceil(S / 2048), W), S entries per window, B buckets per window.  hist: W x B counts (zeroed by the caller).
// The counts of a tile are gathered in LDS first, so that equal keys (every scalar equal: a whole window in one bucket) cost one
// global atomic per tile instead of one per entry.
__global__ void __launch_bounds__(256) k_kd_msm_hist(const uint32_t* key, size_t S, uint32_t B, uint32_t* hist) {
  __shared__ uint32_t cnt[MSM_LDS_KEYS];
  uint32_t k[MSM_EPL]; size_t idx[MSM_EPL];
  load_tile_keys(key, S, k, idx);
  for (uint32_t r0 = 0; r0 < B; r0 += MSM_LDS_KEYS) {
    const uint32_t nr = B - r0 < MSM_LDS_KEYS ? B - r0 : MSM_LDS_KEYS;
    for (uint32_t t = threadIdx.x; t < nr; t += 256) cnt[t] = 0;
    __syncthreads();
    for (int e = 0; e < MSM_EPL; ++e) if (k[e] - r0 < nr) atomicAdd(&cnt[k[e] - r0], 1u);     // MSM_NO_KEY and keys < r0 wrap past nr
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < nr; t += 256) { const uint32_t v = cnt[t]; if (v) atomicAdd(&hist[(size_t)blockIdx.y * B + r0 + t], v); }
    __syncthreads();
  }
}
// cursor: the bucket starts (k_scan_excl of hist); on return each holds one past its bucket's last entry.  sorted[pos] = the
// entry's value (row << 1 | sign); order within a bucket: arbitrary.
__global__ void __launch_bounds__(256) k_kd_msm_scatter(const uint32_t* key, const uint32_t* val, size_t S, uint32_t B, uint32_t* cursor, uint32_t* sorted) {
  __shared__ uint32_t cnt[MSM_LDS_KEYS];
  uint32_t k[MSM_EPL], rank[MSM_EPL]; size_t idx[MSM_EPL];
  load_tile_keys(key, S, k, idx);
  for (uint32_t r0 = 0; r0 < B; r0 += MSM_LDS_KEYS) {
    const uint32_t nr = B - r0 < MSM_LDS_KEYS ? B - r0 : MSM_LDS_KEYS;
    for (uint32_t t = threadIdx.x; t < nr; t += 256) cnt[t] = 0;
    __syncthreads();
    for (int e = 0; e < MSM_EPL; ++e) rank[e] = k[e] - r0 < nr ? atomicAdd(&cnt[k[e] - r0], 1u) : 0u;
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < nr; t += 256) { const uint32_t v = cnt[t]; if (v) cnt[t] = atomicAdd(&cursor[(size_t)blockIdx.y * B + r0 + t], v); }   // count -> base
    __syncthreads();
    for (int e = 0; e < MSM_EPL; ++e) if (k[e] - r0 < nr) sorted[cnt[k[e] - r0] + rank[e]] = val[idx[e]];
    __syncthreads();
  }
}

// ---------------------------------------------------------------- bucket sums, reduction, final combination
BN_KERNEL k_msm_g1_bucket(uint32_t nslots, int level, int final_level, const uint32_t* hist, const uint32_t* run_end, uint32_t u, const uint32_t* sorted,
                          const int32_t* pts, size_t rows, const int32_t* in_ws, size_t in_st, int32_t* out_ws, size_t out_st) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nslots) return;
  msm_bucket_lane<Fp>(s, level, final_level != 0, hist, run_end, u, sorted, pts, rows, in_ws, in_st, out_ws, out_st);
}
BN_KERNEL k_msm_g2_bucket(uint32_t nslots, int level, int final_level, const uint32_t* hist, const uint32_t* run_end, uint32_t u, const uint32_t* sorted,
                          const int32_t* pts, size_t rows, const int32_t* in_ws, size_t in_st, int32_t* out_ws, size_t out_st) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nslots) return;
  msm_bucket_lane<Fp2>(s, level, final_level != 0, hist, run_end, u, sorted, pts, rows, in_ws, in_st, out_ws, out_st);
}
BN_KERNEL k_msm_g1_reduce(uint32_t W, uint32_t B, uint32_t G, int c, const int32_t* bsum, size_t u, int32_t* seg) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= W * G) return;
  msm_reduce_lane<Fp>(q / G, q % G, B, G, c, bsum, u, seg, (size_t)W * G);
}
BN_KERNEL k_msm_g2_reduce(uint32_t W, uint32_t B, uint32_t G, int c, const int32_t* bsum, size_t u, int32_t* seg) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= W * G) return;
  msm_reduce_lane<Fp2>(q / G, q % G, B, G, c, bsum, u, seg, (size_t)W * G);
}
__global__ void __launch_bounds__(256) k_msm_g1_final(const int32_t* seg, uint32_t W, uint32_t G, int c, const uint32_t* hist, uint32_t u, uint8_t* out, uint32_t* stats) {
  msm_final<Fp>(seg, W, G, c, hist, u, out, stats);
}
__global__ void __launch_bounds__(256) k_msm_g2_final(const int32_t* seg, uint32_t W, uint32_t G, int c, const uint32_t* hist, uint32_t u, uint8_t* out, uint32_t* stats) {
  msm_final<Fp2>(seg, W, G, c, hist, u, out, stats);
}
