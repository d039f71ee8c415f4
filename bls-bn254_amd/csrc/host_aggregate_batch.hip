// host_aggregate_batch.hip -- aggregate verify over ragged groups of (key, message) pairs: bit g = blsbn254_aggregate_verify on
// group g alone, for many groups in one call.  Host side of include/blsbn254.h; kernels in k_aggregate_batch.hip; see host_common.h.
//
// Everything stays on the device between the upload and the bitmap's download.  The N pairs are hashed into slots 0 .. N - 1 of
// one H workspace, the G signatures are placed behind them (slot N + g), the caller's N keys get the r-torsion test.  Then the
// Miller loops run two slots per lane sharing one f^2 (k_miller_hpk2r, the loop of k_miller_hpk2): group g of k pairs takes
// ceil((k + 1) / 2) consecutive lanes over the slot sequence [its pairs ..., its signature], the signature's slot pairing with
// the constant -G2gen.  The lanes are the "items" of the planner the pairing-product equations use (plan_launches_cut): launches
// of at most ctx->chunk lanes cut at a group boundary where one lies in the window, a group cut by a launch boundary carried, each
// group's lanes multiplied level by level (seg_run_levels with k_fp12_seg_prod) with the validity byte folded per lane (k_agb_fold); the products
// then finish as blsbn254_pairing_check_batch's do (final exponentiation, mode 0 bitmap).  Slot and chunk descriptors are
// planned on the host from the offsets and uploaded once.
#include "host_common.h"

extern "C" {

int agg_msg_args(blsbn254_ctx* c, const uint8_t* msgs, const uint64_t* off, const uint64_t* grp_off, size_t n_groups, const uint8_t* dst, size_t dst_len,
                 bool missing, bool pair_missing, const char* call) {
  if (!c) return BLSBN254_E_ARG;
  if (n_groups == 0) return CK_NOTHING;
  if (!grp_off || missing || (dst_len && !dst)) return BLSBN254_E_ARG;
  if (check_offsets(grp_off, n_groups)) { c->last_error = "group offsets decrease"; return BLSBN254_E_ARG; }
  const size_t G = n_groups, base = (size_t)grp_off[0], N = (size_t)(grp_off[G] - grp_off[0]);
  if (N && (pair_missing || !off)) return BLSBN254_E_ARG;
  if (N > MAX_LANES || G > MAX_LANES || N + G > MAX_LANES) {
    c->last_error = std::string("more than 2^23 pairs (the signatures' pairs counted) in one ") + call + " call";
    return BLSBN254_E_ARG;
  }
  if (N && check_offsets(off + base, N)) { c->last_error = "message offsets decrease"; return BLSBN254_E_ARG; }
  if (N && !msgs && off[base + N] != off[base]) return BLSBN254_E_ARG;
  return 0;
}
int agg_batch_args(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, const uint64_t* grp_off, const uint8_t* agg_sigs,
                   size_t n_groups, const uint8_t* dst, size_t dst_len, const uint8_t* valid_bitmap, const char* call) {
  return agg_msg_args(c, msgs, off, grp_off, n_groups, dst, dst_len, !agg_sigs || !valid_bitmap, !pks, call);
}
// The call behind its entry points.  want_dup (blsbn254_aggregate_verify_batch_distinct, and the RLC form's exact route): the
// distinct-message stage runs on the hash points behind the hashing launch and leaves the groups' repeat bits in c->md.h_bits;
// without it the launch sequence, the results and the counters are what they were before the stage existed.
int aggregate_verify_batch_impl(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, const uint64_t* grp_off,
                                const uint8_t* agg_sigs, size_t n_groups, const uint8_t* dst, size_t dst_len, uint8_t* valid_bitmap, bool want_dup,
                                const char* call) {
  const int args = agg_batch_args(c, pks, msgs, off, grp_off, agg_sigs, n_groups, dst, dst_len, valid_bitmap, call);
  if (args) return args == CK_NOTHING ? 0 : args;
  const size_t G = n_groups, base = (size_t)grp_off[0], N = (size_t)(grp_off[G] - grp_off[0]);
  ENTER(c);                                             // settles pending asynchronous verify calls BEFORE the tag is staged
  if (N == 0) {                                         // every group is empty: invalid, as the single call's n == 0 (nothing to launch)
    std::memset(valid_bitmap, 0, (G + 7) / 8);
    c->agb.stat[0] += G;
    if (want_dup) { c->md.h_bits.assign((G + 7) / 8, 0); ++c->md.stat[0]; c->md.stat[3] = 0; }      // ... and none is repeated
    return 0;
  }
  uint32_t dl = 0;
  TRY(stage_dst(c, dst, dst_len, &dl));
  TRY(stage_msgs(c, msgs, off + base, N));

  // lanes: group g's slot sequence [base-relative pairs ..., N + g] two by two
  AgbWs& a = c->agb;
  PcWs& w = c->pc;
  std::vector<uint32_t> &sa = a.h_slot_a, &sb = a.h_slot_b;
  std::vector<uint64_t> lane_off(G + 1);
  sa.clear(); sb.clear();
  sa.reserve((N + G) / 2 + G); sb.reserve((N + G) / 2 + G);
  lane_off[0] = 0;
  for (size_t g = 0; g < G; ++g) {
    const size_t p0 = (size_t)grp_off[g] - base, k = (size_t)(grp_off[g + 1] - grp_off[g]);
    for (size_t j = 0; j <= k; j += 2) {                // positions j, j + 1 of the k + 1 slots
      sa.push_back((uint32_t)(j < k ? p0 + j : N + g));
      sb.push_back(j + 1 < k ? (uint32_t)(p0 + j + 1) : (j + 1 == k ? (uint32_t)(N + g) : AGB_NO_SLOT));
    }
    lane_off[g + 1] = sa.size();
  }
  const size_t lanes = sa.size();
  w.seg.h_start.clear(); w.seg.h_len.clear();
  std::vector<SegLaunch> launches;
  size_t items_max;
  if (!plan_launches_cut(lane_off, G, c->chunk, FP12_SEG_GROUP, launches, w.seg.h_start, w.seg.h_len, &items_max)) {
    c->last_error = "internal: segmented products do not converge";
    return BLSBN254_E_HIP;
  }
  const size_t m_max = std::min(lanes, c->chunk), S = N + G;
  TRY(pc_reserve_products(c, G, items_max));
  TRY(stage_group_offsets(c, a.goff, grp_off, G));
  HIPCHK(c, w.pair_ok.reserve(m_max + 1)); HIPCHK(c, a.sig_ok.reserve(G));
  HIPCHK(c, c->in_a.reserve(128 * N)); HIPCHK(c, c->in_b.reserve(64 * G)); HIPCHK(c, c->h_ws.reserve(S * 18 * 4));
  HIPCHK(c, c->f_ws.reserve(m_max * 108 * 4)); HIPCHK(c, c->q_ws.reserve(m_max * 72 * 4)); HIPCHK(c, c->flags.reserve(N)); HIPCHK(c, c->sub_ok.reserve(N));
  HIPCHK(c, hipMemcpyAsync(c->in_a.p, pks + 128 * base, 128 * N, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->in_b.p, agg_sigs, 64 * G, hipMemcpyHostToDevice, c->stream));
  TRY(upload(c, a.slot_a, sa.data(), 4 * lanes));
  TRY(upload(c, a.slot_b, sb.data(), 4 * lanes));

  const uint8_t* d_pks = (const uint8_t*)c->in_a.p;
  int32_t* h = (int32_t*)c->h_ws.p;
  TRY(launch_hash_to_g1(c, c->stream, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, N, dl, h, S,
             (uint8_t*)nullptr, 0));
  if (want_dup) TRY(msg_distinct_stage(c, h, S, N, MD_AFFINE, (const uint32_t*)a.goff.d.p, G));      // slots 0 .. N - 1: the pairs' points, affine
  TRY(launch(c, c->stream, "agb_place_sigs", grid_lanes(G), k_agb_place_sigs, (const uint8_t*)c->in_b.p, G, h, N, S, (uint8_t*)a.sig_ok.p));
  TRY(launch(c, c->stream, "g2_check", grid_lanes(N), k_g2_check, d_pks, N, (uint8_t*)c->sub_ok.p, (uint8_t*)nullptr));   // the caller's keys only: never -G2gen
  const uint32_t *d_sa = (const uint32_t*)a.slot_a.p, *d_sb = (const uint32_t*)a.slot_b.p;
  for (const SegLaunch& L : launches) {
    const size_t m = L.hi - L.lo;                       // (every group has its signature's lane: no launch is empty)
    TRY(launch(c, c->stream, "miller_hpk2r", grid_lanes(m), k_miller_hpk2r, (const int32_t*)h, S, d_pks, N, d_sa + L.lo, d_sb + L.lo, m, (int32_t*)c->q_ws.p,
               (int32_t*)c->f_ws.p, m, (uint8_t*)c->flags.p));
    TRY(launch(c, c->stream, "agb_fold", grid_lanes(m), k_agb_fold, d_sa + L.lo, d_sb + L.lo, m, N, (const uint8_t*)c->flags.p, (const uint8_t*)c->sub_ok.p,
               (const uint8_t*)a.sig_ok.p, (const uint32_t*)a.goff.d.p, (uint8_t*)w.pair_ok.p));
    TRY(seg_run_levels(w.seg, L.levels, {(const int32_t*)c->f_ws.p, m, (const uint8_t*)w.pair_ok.p}, {(int32_t*)w.prod.p + L.ga, G, (uint8_t*)w.ok.p + L.ga},
                       [&](SegSrc in, const uint32_t* start, const uint32_t* len, size_t runs, SegDst out, bool last) {
      return launch(c, c->stream, "fp12_seg_prod", grid_lanes(runs), k_fp12_seg_prod, in.v, in.stride, in.ok, start, len, runs, out.v, out.stride, out.ok,
                    (last && L.carry) ? 1 : 0);
    }));
  }
  TRY(pc_finish_bitmap(c, G, valid_bitmap));
  if (want_dup) TRY(msg_distinct_bits(c, N, G, nullptr));
  c->agb.stat[0] += G; c->agb.stat[1] += lanes; c->agb.stat[3] += launches.size();      // counted once the call has succeeded
  return 0;
}
int blsbn254_aggregate_verify_batch(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, const uint64_t* grp_off,
                                    const uint8_t* agg_sigs, size_t n_groups, const uint8_t* dst, size_t dst_len, uint8_t* valid_bitmap) {
  return aggregate_verify_batch_impl(c, pks, msgs, off, grp_off, agg_sigs, n_groups, dst, dst_len, valid_bitmap, false, "aggregate_verify_batch");
}

int blsbn254_aggregate_batch_stats(blsbn254_ctx* c, uint64_t out[4]) { return COPY_STATS(c, agb.stat, 4, out); }

}  // extern "C"
