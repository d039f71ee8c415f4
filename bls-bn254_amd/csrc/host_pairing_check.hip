// host_pairing_check.hip -- pairing-product equations over ragged groups of pairs: multi_miller_loop over each group
// (pairings.rs:808-857) and the check prod_j e(P_j, Q_j) == 1 (multi_miller_loop(..).final_exponentiation() == Gt::identity,
// pairings.rs:706-713 with :698-704).  Host side of include/blsbn254.h; kernels in k_pairing_check.hip; see host_common.h.
//
// The pairs run in launches of at most ctx->chunk pairs, cut at an equation boundary where one lies in the window: the Miller
// loops (miller_to_ws, the same wide / tri / lane forms as pairing_batch), the validity fold (check path), then the segmented
// product of each equation's Miller values, level by level as k_g2_seg_sum, the last level writing straight into the
// per-equation products (limb-major, stride n_eq).  An equation cut by a launch boundary is carried: the next launch's first
// chunk multiplies into its running product.  Then the products go through the final exponentiation (mode 0 bitmap) in chunks
// of ctx->chunk equations, or to bytes.  All chunk descriptors are planned on the host up front and uploaded in one copy.
#include "host_common.h"

extern "C" {

static const size_t FP12_SEG_GROUP = 8;     // Miller values per lane of the segmented product

// Launches and their product levels for equations rel[0..n_eq] (offsets rebased to 0); descriptors appended to start / len.
int pc_plan_launches(blsbn254_ctx* c, const std::vector<uint64_t>& rel, size_t n_eq, std::vector<PcLaunch>& out,
                     std::vector<uint32_t>& start, std::vector<uint32_t>& len, size_t* items_max) {
  const size_t N = (size_t)rel[n_eq];
  size_t lo = 0, g = 0;
  *items_max = 1;
  do {
    PcLaunch L;
    const size_t lim = std::min(N, lo + c->chunk);
    // the last equation boundary in (lo, lim], else lim (inside an equation larger than a chunk)
    const size_t k = (size_t)(std::upper_bound(rel.begin(), rel.end(), (uint64_t)lim) - rel.begin()) - 1;
    const size_t hi = rel[k] > lo ? (size_t)rel[k] : lim;
    // equations [g, gb): the unfinished ones that begin before hi; the last launch takes every remaining (empty) one
    const size_t gb = hi == N ? n_eq : (size_t)(std::lower_bound(rel.begin(), rel.end(), (uint64_t)hi) - rel.begin());
    L.lo = lo; L.hi = hi; L.ga = g; L.gb = gb; L.carry = rel[g] < lo;
    const size_t ne = gb - g;
    std::vector<uint64_t> cur(ne + 1);
    for (size_t e = 0; e <= ne; ++e) cur[e] = std::min<uint64_t>(std::max<uint64_t>(rel[g + e], lo), hi) - lo;   // launch-local boundaries
    TRY(plan_seg_levels(c, cur, FP12_SEG_GROUP, start, len, L.levels, "internal: segmented products do not converge"));
    for (size_t lv = 0; lv + 1 < L.levels.size(); ++lv) *items_max = std::max(*items_max, L.levels[lv].count);   // (the last level writes into the products)
    out.push_back(std::move(L));
    g = (gb > g && rel[gb] > hi) ? gb - 1 : gb;      // an equation cut at hi continues in the next launch
    lo = hi;
  } while (lo < N);
  return 0;
}

// The products' buffers: per-equation products and flags, the levels' ping-pong items (items_max of pc_plan_launches)
int pc_reserve_products(blsbn254_ctx* c, size_t n_eq, size_t items_max) {
  PcWs& w = c->pc;
  HIPCHK(c, w.prod.reserve(n_eq * 108 * 4)); HIPCHK(c, w.ok.reserve(n_eq));
  HIPCHK(c, w.seg[0].reserve(items_max * 108 * 4)); HIPCHK(c, w.seg[1].reserve(items_max * 108 * 4));
  HIPCHK(c, w.seg_ok[0].reserve(items_max)); HIPCHK(c, w.seg_ok[1].reserve(items_max));
  return 0;
}
// One launch's product levels: its items' values at src (limb-major, src_stride; nullptr for a launch of empty equations) and,
// with `check`, their flags at src_ok, into the products / flags of equations L.ga .. L.gb (stride n_eq).  The descriptors are
// c->pc.start / len, uploaded by the caller.
int pc_run_levels(blsbn254_ctx* c, const PcLaunch& L, const int32_t* src, const uint8_t* src_ok, size_t src_stride, size_t n_eq, bool check) {
  PcWs& w = c->pc;
  int dst = 0;
  for (size_t lv = 0; lv < L.levels.size(); ++lv) {
    const SegLevel& P = L.levels[lv];
    const bool last = lv + 1 == L.levels.size();
    int32_t* out = last ? (int32_t*)w.prod.p + L.ga : (int32_t*)w.seg[dst].p;
    uint8_t* out_ok = check ? (last ? (uint8_t*)w.ok.p + L.ga : (uint8_t*)w.seg_ok[dst].p) : nullptr;
    TRY(launch(c, c->stream, "fp12_seg_prod", grid_lanes(P.count), k_fp12_seg_prod, src, src_stride, src_ok, (const uint32_t*)w.start.p + P.first,
               (const uint32_t*)w.len.p + P.first, P.count, out, last ? n_eq : P.count, out_ok, (last && L.carry) ? 1 : 0));
    src = out; src_ok = out_ok; src_stride = P.count; dst ^= 1;
  }
  return 0;
}

// Products of every equation into c->pc.prod (limb-major, stride n_eq) and, with `check`, their validity into c->pc.ok.
static int pc_products(blsbn254_ctx* c, const uint8_t* g1, const uint8_t* g2, const uint64_t* off, size_t n_eq, bool check) {
  const size_t N = (size_t)(off[n_eq] - off[0]);
  std::vector<uint64_t> rel(n_eq + 1);
  for (size_t g = 0; g <= n_eq; ++g) rel[g] = off[g] - off[0];
  PcWs& w = c->pc;
  std::vector<uint32_t>& start = w.h_start;           // ctx-owned: outlive the asynchronous copies (every call ends synchronised)
  std::vector<uint32_t>& len = w.h_len;
  start.clear(); len.clear();
  std::vector<PcLaunch> launches;
  size_t items_max;
  int rc = pc_plan_launches(c, rel, n_eq, launches, start, len, &items_max);
  if (rc) return rc;
  TRY(pc_reserve_products(c, n_eq, items_max));
  HIPCHK(c, w.start.reserve(4 * start.size())); HIPCHK(c, w.len.reserve(4 * len.size()));
  HIPCHK(c, c->in_a.reserve(64 * (N ? N : 1))); HIPCHK(c, c->in_b.reserve(128 * (N ? N : 1)));
  if (check) HIPCHK(c, w.pair_ok.reserve(std::min(N, c->chunk) + 1));
  if (N) {
    HIPCHK(c, hipMemcpyAsync(c->in_a.p, g1 + 64 * off[0], 64 * N, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->in_b.p, g2 + 128 * off[0], 128 * N, hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, hipMemcpyAsync(w.start.p, start.data(), 4 * start.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(w.len.p, len.data(), 4 * len.size(), hipMemcpyHostToDevice, c->stream));
  const uint8_t *d_g1 = (const uint8_t*)c->in_a.p, *d_g2 = (const uint8_t*)c->in_b.p;
  for (const PcLaunch& L : launches) {
    const size_t m = L.hi - L.lo;
    const int32_t* src = nullptr;                     // level 0 reads the launch's Miller values (none for a launch of empty equations)
    const uint8_t* src_ok = check ? (const uint8_t*)w.pair_ok.p : nullptr;
    size_t src_stride = m ? m : 1;
    if (m) {
      rc = miller_to_ws(c, d_g1 + 64 * L.lo, d_g2 + 128 * L.lo, m);
      if (rc) return rc;
      src = (const int32_t*)c->f_ws.p;
      if (check) {
        TRY(launch(c, c->stream, "pair_ok", grid_lanes(m), k_pair_ok, d_g1 + 64 * L.lo, d_g2 + 128 * L.lo, m, (uint8_t*)w.pair_ok.p));
      } else {                                        // the errors of multi_miller_loop: the first pair that does not decode
        int bad;
        rc = first_bad(c, (const uint8_t*)c->status.p, m, 3, 3, &bad);
        if (rc) return rc;
        if (bad >= 0) {
          uint8_t st = 0;
          rc = read_status(c, (const uint8_t*)c->status.p, bad, &st);
          if (rc) return rc;
          c->last_error = std::string(st & 1 ? "G2" : "G1") + " point does not decode at pair " + std::to_string((size_t)off[0] + L.lo + (size_t)bad);
          return (st & 1) ? BLSBN254_ERR_G2 : BLSBN254_ERR_G1;
        }
      }
    }
    rc = pc_run_levels(c, L, src, src_ok, src_stride, n_eq, check);
    if (rc) return rc;
  }
  return 0;
}

static int pc_args(blsbn254_ctx* c, const uint8_t* g1, const uint8_t* g2, const uint64_t* off, size_t n_eq, const void* out) {
  if (!off || !out) return BLSBN254_E_ARG;
  if (check_offsets(off, n_eq)) { c->last_error = "equation offsets decrease"; return BLSBN254_E_ARG; }
  const size_t N = (size_t)(off[n_eq] - off[0]);
  if (N && (!g1 || !g2)) return BLSBN254_E_ARG;
  CHECK_LANES(c, N);
  CHECK_LANES(c, n_eq);
  return 0;
}

int blsbn254_multi_miller_loop_batch(blsbn254_ctx* c, const uint8_t* g1, const uint8_t* g2, const uint64_t* off, size_t n_eq, uint8_t* ml_out) {
  if (!c) return BLSBN254_E_ARG;
  if (n_eq == 0) return 0;
  int rc = pc_args(c, g1, g2, off, n_eq, ml_out);
  if (rc) return rc;
  ENTER(c);
  rc = pc_products(c, g1, g2, off, n_eq, false);
  if (rc) return rc;
  HIPCHK(c, c->out.reserve(384 * n_eq));
  TRY(launch(c, c->stream, "fp12_to_bytes", grid_lanes(n_eq), k_fp12_to_bytes, (const int32_t*)c->pc.prod.p, n_eq, n_eq, (uint8_t*)c->out.p));
  return download(c, ml_out, c->out.p, 384 * n_eq);
}

int blsbn254_pairing_check_batch(blsbn254_ctx* c, const uint8_t* g1, const uint8_t* g2, const uint64_t* off, size_t n_eq, uint8_t* valid_bitmap) {
  if (!c) return BLSBN254_E_ARG;
  if (n_eq == 0) return 0;
  int rc = pc_args(c, g1, g2, off, n_eq, valid_bitmap);
  if (rc) return rc;
  ENTER(c);
  rc = pc_products(c, g1, g2, off, n_eq, true);
  if (rc) return rc;
  return pc_finish_bitmap(c, n_eq, valid_bitmap);
}
// The final exponentiation of the n_eq products in c->pc.prod with their flags c->pc.ok (mode 0), and the bitmap's download
int pc_finish_bitmap(blsbn254_ctx* c, size_t n_eq, uint8_t* valid_bitmap) {
  const size_t nb = (n_eq + 7) / 8;
  HIPCHK(c, c->bitmap.reserve(nb + 8));
  int32_t* prod = (int32_t*)c->pc.prod.p;
  const uint8_t* ok = (const uint8_t*)c->pc.ok.p;
  // chunks of ctx->chunk equations (a multiple of 8: whole bitmap bytes); beyond one chunk each is first gathered into f_ws
  // (the Miller values are consumed) so that the final exponentiation keeps stride == n
  TRY(for_chunks(c, n_eq, [&](size_t e0, size_t m) -> int {
    int32_t* f = prod;
    if (m != n_eq) {
      HIPCHK(c, c->f_ws.reserve(m * 108 * 4));
      f = (int32_t*)c->f_ws.p;
      HIPCHK(c, hipMemcpy2DAsync(f, m * 4, prod + e0, n_eq * 4, m * 4, 108, hipMemcpyDeviceToDevice, c->stream));
    }
    return run_final_exp(c, f, m, m, 0, ok + e0, ok + e0, (uint8_t*)c->bitmap.p + e0 / 8, nullptr, nullptr);
  }));
  return download(c, valid_bitmap, c->bitmap.p, nb);
}

}  // extern "C"
