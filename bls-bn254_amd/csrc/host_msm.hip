// host_msm.hip -- multi-scalar multiplication out = sum_i [k_i] P_i for G1 and G2 (LinearCombination, n-term form) by the bucket
// method.  Host side of include/blsbn254.h; kernels in k_msm_bucket.hip, the per-lane arithmetic in msm.h (algorithm there).
// Every phase is one launch on the context's stream; the only read-backs are the status reduction and the result.
#include "host_common.h"
#include "msm.h"

BN_KERNEL k_msm_g1_prep(const uint8_t* g1, const uint8_t* scalars, size_t n, int c, int W, int32_t* pts, uint32_t* key, uint32_t* val, uint8_t* status);
BN_KERNEL k_msm_g2_prep(const uint8_t* g2, const uint8_t* scalars, size_t n, int c, int W, int32_t* pts, uint32_t* key, uint32_t* val, uint8_t* status);
__global__ void __launch_bounds__(256) k_kd_msm_hist(const uint32_t* key, size_t S, uint32_t B, uint32_t* hist);
__global__ void __launch_bounds__(256) k_kd_msm_scatter(const uint32_t* key, const uint32_t* val, size_t S, uint32_t B, uint32_t* cursor, uint32_t* sorted);
BN_KERNEL k_msm_g1_bucket(uint32_t nslots, int level, int final_level, const uint32_t* hist, const uint32_t* run_end, uint32_t u, const uint32_t* sorted,
                          const int32_t* pts, size_t rows, const int32_t* in_ws, size_t in_st, int32_t* out_ws, size_t out_st);
BN_KERNEL k_msm_g2_bucket(uint32_t nslots, int level, int final_level, const uint32_t* hist, const uint32_t* run_end, uint32_t u, const uint32_t* sorted,
                          const int32_t* pts, size_t rows, const int32_t* in_ws, size_t in_st, int32_t* out_ws, size_t out_st);
BN_KERNEL k_msm_g1_reduce(uint32_t W, uint32_t B, uint32_t G, int c, const int32_t* bsum, size_t u, int32_t* seg);
BN_KERNEL k_msm_g2_reduce(uint32_t W, uint32_t B, uint32_t G, int c, const int32_t* bsum, size_t u, int32_t* seg);
__global__ void __launch_bounds__(256) k_msm_g1_final(const int32_t* seg, uint32_t W, uint32_t G, int c, const uint32_t* hist, uint32_t u, uint8_t* out, uint32_t* stats);
__global__ void __launch_bounds__(256) k_msm_g2_final(const int32_t* seg, uint32_t W, uint32_t G, int c, const uint32_t* hist, uint32_t u, uint8_t* out, uint32_t* stats);

namespace {
const size_t MSM_MAX_N = (size_t)1 << 23;
const int MSM_SORT_TILE = 2048;        // k_kd_msm_* entries per workgroup

// window width from n: minimise W(c) (entries per window + 1.5 x the 2 additions per bucket of the reduction), c in 2..16
int msm_choose_window(size_t n, int halves, int bits) {
  int best = 2; double best_cost = 0;
  for (int c = 2; c <= 16; ++c) {
    const double cost = (double)msm_windows(bits, c) * ((double)halves * (double)n + 1.5 * (double)(1u << c));
    if (c == 2 || cost < best_cost) { best = c; best_cost = cost; }
  }
  return best;
}

int msm_common(blsbn254_ctx* c, const uint8_t* pts, const uint8_t* scalars, size_t n, uint8_t* out, int g2) {
  const size_t psz = g2 ? 128 : 64;
  if (!c || !out || (n && (!pts || !scalars))) return BLSBN254_E_ARG;
  if (n == 0) { std::memset(out, 0, psz); out[psz - 1] = 1; return 0; }          // the identity encoding: x = 0, y = 1
  if (n > MSM_MAX_N) { c->last_error = "more than 2^23 terms in one multi-scalar multiplication"; return BLSBN254_E_ARG; }
  ENTER(c);
  const int halves = g2 ? 1 : 2, bits = g2 ? 254 : 128, K = g2 ? 2 * NL : NL;      // G1: GLV halves of <= 128 bits
  const int cw = c->msm_window ? c->msm_window : msm_choose_window(n, halves, bits);
  const uint32_t W = (uint32_t)msm_windows(bits, cw), B = 1u << (cw - 1), u = W * B;
  const size_t S = (size_t)halves * n, E = S * W;                                   // entries per window, entry slots
  const uint32_t G = B < (uint32_t)MSM_MAX_SEGS ? B : (uint32_t)MSM_MAX_SEGS;
  int levels = 0;                                                                   // chunk levels before the last: L^(levels+1) >= S
  while (((size_t)1 << (MSM_LG_CHUNK * (levels + 1))) < S) ++levels;
  const size_t slots0 = (E >> MSM_LG_CHUNK) + u + 1;                               // level-0 output slots (msm.h: off_0 bound)
  MsmWs& m = c->msm;
  HIPCHK(c, c->status.reserve(n)); HIPCHK(c, c->out.reserve(psz));
  HIPCHK(c, m.pts.reserve(S * 2 * K * 4)); HIPCHK(c, m.key.reserve(E * 4)); HIPCHK(c, m.val.reserve(E * 4)); HIPCHK(c, m.sorted.reserve(E * 4));
  HIPCHK(c, m.hist.reserve((size_t)u * 4)); HIPCHK(c, m.end.reserve((size_t)u * 4));
  HIPCHK(c, m.part[0].reserve(slots0 * 3 * K * 4)); HIPCHK(c, m.part[1].reserve(slots0 * 3 * K * 4));
  HIPCHK(c, m.bsum.reserve((size_t)u * 3 * K * 4)); HIPCHK(c, m.seg.reserve((size_t)W * G * 3 * K * 4)); HIPCHK(c, m.dstat.reserve(8));
  TRY(upload(c, c->in_a, pts, psz * n));
  TRY(upload(c, c->scalars, scalars, 32 * n));
  const uint8_t* d_pts = (const uint8_t*)c->in_a.p; const uint8_t* d_sc = (const uint8_t*)c->scalars.p;
  int32_t* rows = (int32_t*)m.pts.p; uint32_t* key = (uint32_t*)m.key.p; uint32_t* val = (uint32_t*)m.val.p; uint32_t* sorted = (uint32_t*)m.sorted.p;
  uint32_t* hist = (uint32_t*)m.hist.p; uint32_t* end = (uint32_t*)m.end.p;
  uint8_t* status = (uint8_t*)c->status.p;
  if (g2) TRY(launch(c, c->stream, "msm_prep", grid_lanes(n), k_msm_g2_prep, d_pts, d_sc, n, cw, (int)W, rows, key, val, status));
  else TRY(launch(c, c->stream, "msm_prep", grid_lanes(n), k_msm_g1_prep, d_pts, d_sc, n, cw, (int)W, rows, key, val, status));
  // counting sort by (window, bucket)
  const dim3 sort_grid((unsigned)((S + MSM_SORT_TILE - 1) / MSM_SORT_TILE), W);
  HIPCHK(c, hipMemsetAsync(hist, 0, (size_t)u * 4, c->stream));
  TRY(launch(c, c->stream, "msm_hist", Shape{sort_grid, dim3(256)}, k_kd_msm_hist, (const uint32_t*)key, S, B, hist));
  TRY(launch(c, c->stream, "msm_scan", Shape{dim3(1), dim3(1024)}, k_scan_excl, (const uint32_t*)hist, u, end));
  TRY(launch(c, c->stream, "msm_scatter", Shape{sort_grid, dim3(256)}, k_kd_msm_scatter, (const uint32_t*)key, (const uint32_t*)val, S, B, end, sorted));
  // bucket sums: levels 0 .. levels-1 into the ping-pong slots, the last level into bsum (slot = bucket)
  const int32_t* in_ws = nullptr; size_t in_st = 1;
  for (int lv = 0; lv <= levels; ++lv) {
    const bool fin = lv == levels;
    const size_t nslots = fin ? (size_t)u : (E >> (MSM_LG_CHUNK * (lv + 1))) + u + 1;
    int32_t* out_ws = fin ? (int32_t*)m.bsum.p : (int32_t*)m.part[lv & 1].p;
    if (g2) TRY(launch(c, c->stream, "msm_bucket", grid_lanes(nslots), k_msm_g2_bucket, (uint32_t)nslots, lv, fin ? 1 : 0, (const uint32_t*)hist, (const uint32_t*)end, u,
                       (const uint32_t*)sorted, (const int32_t*)rows, S, in_ws, in_st, out_ws, nslots));
    else TRY(launch(c, c->stream, "msm_bucket", grid_lanes(nslots), k_msm_g1_bucket, (uint32_t)nslots, lv, fin ? 1 : 0, (const uint32_t*)hist, (const uint32_t*)end, u,
                    (const uint32_t*)sorted, (const int32_t*)rows, S, in_ws, in_st, out_ws, nslots));
    in_ws = out_ws; in_st = nslots;
  }
  const size_t lanes = (size_t)W * G;
  if (g2) TRY(launch(c, c->stream, "msm_reduce", grid_lanes(lanes), k_msm_g2_reduce, W, B, G, cw, (const int32_t*)m.bsum.p, (size_t)u, (int32_t*)m.seg.p));
  else TRY(launch(c, c->stream, "msm_reduce", grid_lanes(lanes), k_msm_g1_reduce, W, B, G, cw, (const int32_t*)m.bsum.p, (size_t)u, (int32_t*)m.seg.p));
  if (g2) TRY(launch(c, c->stream, "msm_final", grid_lanes(1), k_msm_g2_final, (const int32_t*)m.seg.p, W, G, cw, (const uint32_t*)hist, u, (uint8_t*)c->out.p, (uint32_t*)m.dstat.p));
  else TRY(launch(c, c->stream, "msm_final", grid_lanes(1), k_msm_g1_final, (const int32_t*)m.seg.p, W, G, cw, (const uint32_t*)hist, u, (uint8_t*)c->out.p, (uint32_t*)m.dstat.p));
  // the validity of every term (first bad index, as blsbn254_g1_mul_batch)
  int bad;
  int rc = first_bad(c, status, n, 3, 3, &bad);
  if (rc) return rc;
  if (bad >= 0) {
    uint8_t st = 0;
    rc = read_status(c, status, bad, &st);
    if (rc) return rc;
    c->last_error = std::string(st & 1 ? "scalar not canonical" : "point does not decode or is off the curve") + " at element " + std::to_string((size_t)bad);
    return (st & 1) ? BLSBN254_ERR_SCALAR : (g2 ? BLSBN254_ERR_G2 : BLSBN254_ERR_G1);
  }
  uint32_t cnt[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(out, c->out.p, psz, hipMemcpyDeviceToHost, c->stream));
  TRY(download(c, cnt, m.dstat.p, 8));
  c->msm.stat[0] += 1; c->msm.stat[2] += cnt[0]; c->msm.stat[3] += cnt[1];
  return 0;
}
}  // namespace

extern "C" {

int blsbn254_g1_msm(blsbn254_ctx* c, const uint8_t* g1, const uint8_t* scalars, size_t n, uint8_t out[64]) { return msm_common(c, g1, scalars, n, out, 0); }
int blsbn254_g2_msm(blsbn254_ctx* c, const uint8_t* g2, const uint8_t* scalars, size_t n, uint8_t out[128]) { return msm_common(c, g2, scalars, n, out, 1); }
int blsbn254_set_msm_window(blsbn254_ctx* c, int cw) {
  if (!c || (cw != 0 && (cw < 2 || cw > 16))) return BLSBN254_E_ARG;
  c->msm_window = cw;
  return 0;
}
int blsbn254_msm_stats(blsbn254_ctx* c, uint64_t out[4]) { return COPY_STATS(c, msm.stat, 4, out); }

}  // extern "C"
