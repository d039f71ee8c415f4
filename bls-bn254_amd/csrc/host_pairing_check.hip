// host_pairing_check.hip -- pairing-product equations over ragged groups of pairs: multi_miller_loop over each group
// (pairings.rs:808-857) and the check prod_j e(P_j, Q_j) == 1 (multi_miller_loop(..).final_exponentiation() == Gt::identity,
// pairings.rs:706-713 with :698-704).  Host side of include/blsbn254.h; kernels in k_pairing_check.hip; see host_common.h.
//
// The pairs run in launches of at most ctx->chunk pairs, cut at an equation boundary where one lies in the window: the Miller
// loops (miller_to_ws, the same wide / tri / lane forms as pairing_batch), the validity fold (check path), then the segmented
// product of each equation's Miller values, level by level (seg_run_levels with k_fp12_seg_prod), the last level writing
// straight into the per-equation products (limb-major, stride n_eq).  An equation cut by a launch boundary is carried: the next
// launch's first chunk multiplies into its running product.  Then the products go through the final exponentiation (mode 0
// bitmap) in chunks of ctx->chunk equations, or to bytes.  All launches and their levels are planned on the host up front
// (plan_launches_cut, seg_plan.h) and the descriptors uploaded in one copy.
#include "host_common.h"

extern "C" {

// The products' buffers: per-equation products and flags, and c->pc.seg staged for the launches planned into its host copies
// (items_max of plan_launches_cut)
int pc_reserve_products(blsbn254_ctx* c, size_t n_eq, size_t items_max) {
  PcWs& w = c->pc;
  HIPCHK(c, w.prod.reserve(n_eq * 108 * 4)); HIPCHK(c, w.ok.reserve(n_eq));
  return seg_stage(c, w.seg, items_max, 108, true);
}

// Products of every equation into c->pc.prod (limb-major, stride n_eq) and, with `check`, their validity into c->pc.ok.
static int pc_products(blsbn254_ctx* c, const uint8_t* g1, const uint8_t* g2, const uint64_t* off, size_t n_eq, bool check) {
  const size_t N = (size_t)(off[n_eq] - off[0]);
  std::vector<uint64_t> rel(n_eq + 1);
  for (size_t g = 0; g <= n_eq; ++g) rel[g] = off[g] - off[0];
  PcWs& w = c->pc;
  w.seg.h_start.clear(); w.seg.h_len.clear();
  std::vector<SegLaunch> launches;
  size_t items_max;
  if (!plan_launches_cut(rel, n_eq, c->chunk, FP12_SEG_GROUP, launches, w.seg.h_start, w.seg.h_len, &items_max)) {
    c->last_error = "internal: segmented products do not converge";
    return BLSBN254_E_HIP;
  }
  TRY(pc_reserve_products(c, n_eq, items_max));
  HIPCHK(c, c->in_a.reserve(64 * (N ? N : 1))); HIPCHK(c, c->in_b.reserve(128 * (N ? N : 1)));
  if (check) HIPCHK(c, w.pair_ok.reserve(std::min(N, c->chunk) + 1));
  if (N) {
    HIPCHK(c, hipMemcpyAsync(c->in_a.p, g1 + 64 * off[0], 64 * N, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->in_b.p, g2 + 128 * off[0], 128 * N, hipMemcpyHostToDevice, c->stream));
  }
  const uint8_t *d_g1 = (const uint8_t*)c->in_a.p, *d_g2 = (const uint8_t*)c->in_b.p;
  for (const SegLaunch& L : launches) {
    const size_t m = L.hi - L.lo;
    const int32_t* src = nullptr;                     // level 0 reads the launch's Miller values (none for a launch of empty equations)
    const uint8_t* src_ok = check ? (const uint8_t*)w.pair_ok.p : nullptr;
    size_t src_stride = m ? m : 1;
    if (m) {
      TRY(miller_to_ws(c, d_g1 + 64 * L.lo, d_g2 + 128 * L.lo, m));
      src = (const int32_t*)c->f_ws.p;
      if (check) {
        TRY(launch(c, c->stream, "pair_ok", grid_lanes(m), k_pair_ok, d_g1 + 64 * L.lo, d_g2 + 128 * L.lo, m, (uint8_t*)w.pair_ok.p));
      } else {                                        // the errors of multi_miller_loop: the first pair that does not decode
        int bad;
        TRY(first_bad(c, (const uint8_t*)c->status.p, m, 3, 3, &bad));
        if (bad >= 0) {
          uint8_t st = 0;
          TRY(read_status(c, (const uint8_t*)c->status.p, bad, &st));
          c->last_error = std::string(st & 1 ? "G2" : "G1") + " point does not decode at pair " + std::to_string((size_t)off[0] + L.lo + (size_t)bad);
          return (st & 1) ? BLSBN254_ERR_G2 : BLSBN254_ERR_G1;
        }
      }
    }
    TRY(seg_run_levels(w.seg, L.levels, {src, src_stride, src_ok}, {(int32_t*)w.prod.p + L.ga, n_eq, check ? (uint8_t*)w.ok.p + L.ga : nullptr},
                       [&](SegSrc in, const uint32_t* start, const uint32_t* len, size_t runs, SegDst out, bool last) {
      return launch(c, c->stream, "fp12_seg_prod", grid_lanes(runs), k_fp12_seg_prod, in.v, in.stride, in.ok, start, len, runs, out.v, out.stride, out.ok,
                    (last && L.carry) ? 1 : 0);
    }));
  }
  return 0;
}

int pc_args(blsbn254_ctx* c, const uint8_t* g1, const uint8_t* g2, const uint64_t* off, size_t n_eq, const void* out) {
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
