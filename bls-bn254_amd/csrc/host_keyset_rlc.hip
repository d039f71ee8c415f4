// host_keyset_rlc.hip -- FastAggregateVerify over a registered key set (and over its committees) by random linear combination per
// message: the groups of a call that sign the SAME message are weighed with secret 64-bit scalars and checked a chunk at a time,
//     e(sum_g r_g sig_g, -G2gen) e(H(m), sum_g r_g S_g) == 1,
// one pairing equation for up to C aggregates.  Host side of include/blsbn254.h; kernels in k_keyset_rlc.hip, lane functions in
// keyset_rlc.h, the plan in keyset_rlc_plan.h; see host_common.h and DESIGN.md 6m.
//
// A call: the key sums exactly as the exact calls make them (ks_enqueue_sums / kc_enqueue_call, into c->gs.sum / c->gs.sum_ok); the
// plan (ksr_plan: classes by message bytes, the stable order, chunks, the runs of the sums); k_ksr_elig, the two weight kernels,
// the segmented sums of the weighted points over the chunks (k_g1_seg_sum, k_g2_seg_sum by seg_run_levels), k_ksr_chunks; the
// chunks worth checking go through verify_chunk_dev as virtual tuples (sum B, the class's message, sum A).  An eligible group of a
// chunk that passed has its bit set.  EVERYTHING ELSE -- ineligible groups, chunks with fewer than two eligible members or a sum
// that is the identity, the eligible members of a chunk that failed -- goes to the exact pipeline of ks_verify_sums in ONE
// sub-call on the gathered sums, so every edge case keeps the exact call's bit by construction.
#include "host_common.h"

extern "C" {

// One sub-call of the verify pipeline on the columns w.h_list of pts (54 limbs, stride; flags ok or none) with the signatures
// sigs[64 i] of the same columns and the messages staged in w.h_msgs / w.h_moff: the bits into w.h_bits (synchronised)
static int ksr_subcall(blsbn254_ctx* c, const int32_t* pts, size_t stride, const uint8_t* ok, const uint8_t* sigs, int poison, uint32_t dl) {
  KsrWs& w = c->ksr;
  const size_t m = w.h_list.size(), nb = (m + 7) / 8;
  TRY(upload(c, w.list, w.h_list.data(), 4 * m));
  TRY(upload(c, w.msgs, w.h_msgs.data(), w.h_msgs.size()));         // (h_msgs ends with a spare byte: never empty)
  TRY(upload(c, w.moff, w.h_moff.data(), 8 * (m + 1)));
  HIPCHK(c, w.c_pts.reserve(54 * 4 * m)); HIPCHK(c, w.c_ok.reserve(m)); HIPCHK(c, w.c_sigs.reserve(64 * m));
  HIPCHK(c, w.pk.reserve(128 * m)); HIPCHK(c, w.bits.reserve(nb + 8));
  TRY(launch(c, c->stream, "ksr_gather", grid_lanes(m), k_ksr_gather, (const uint32_t*)w.list.p, m, pts, stride, ok, sigs, (int32_t*)w.c_pts.p, (uint8_t*)w.c_ok.p,
             (uint8_t*)w.c_sigs.p));
  TRY(launch(c, c->stream, "g2p_to_bytes", grid_lanes(m), k_g2p_to_bytes, (const int32_t*)w.c_pts.p, m, (const uint8_t*)w.c_ok.p, m, (uint8_t*)w.pk.p, poison));
  TRY(verify_chunk_dev(c, (const uint8_t*)w.pk.p, (const uint8_t*)w.msgs.p, (const uint64_t*)w.moff.p, (const uint8_t*)w.c_sigs.p, m, dl, (uint8_t*)w.bits.p));
  w.h_bits.resize(nb);
  return download(c, w.h_bits.data(), w.bits.p, nb);
}
// the message of group g behind the messages already in w.h_msgs
static void ksr_push_msg(KsrWs& w, const uint8_t* msgs, const uint64_t* off, size_t g) {
  if (off[g + 1] > off[g]) w.h_msgs.insert(w.h_msgs.end(), msgs + off[g], msgs + off[g + 1]);
  w.h_moff.push_back(w.h_msgs.size());
}

// the signatures into c->in_b and the seed (the caller's, or 32 bytes drawn now: after the batch is fixed) into c->ksr.seed
static int ksr_stage(blsbn254_ctx* c, const uint8_t* sigs, const uint8_t* seed, size_t n) {
  TRY(stage_seed(c, c->ksr.seed, seed));
  return upload(c, c->in_b, sigs, 64 * n);
}

// From the sums on (c->gs.sum / c->gs.sum_ok enqueued, the signatures and the seed staged, the tag resident).  com != nullptr: the
// committee form, rows in c->kcom.sel at sel_off[g] - sel_off[0]; else the rows are in c->kset.sel.
static int ksr_run(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* com, const uint64_t* sel_off, const uint8_t* msgs, const uint64_t* off,
                   size_t n, uint32_t dl, uint8_t* bm) {
  Stream2Guard s2_guard(c);
  KsrWs& w = c->ksr;
  KsrPlan& P = w.plan;
  if (!ksr_plan(msgs, off, n, c->ksr_group, P, w.seg.h_start, w.seg.h_len)) { c->last_error = "internal: chunk sums do not converge"; return BLSBN254_E_HIP; }
  const size_t M = P.chunks.size();
  const uint8_t* d_sigs = (const uint8_t*)c->in_b.p;
  if (!P.n_multi) {                                          // no two groups share a message: the exact call's own tail, nothing to gather
    TRY(stage_msgs(c, msgs, off, n));
    HIPCHK(c, c->gs.pk.reserve(128 * n)); HIPCHK(c, c->bitmap.reserve((n + 7) / 8 + 8));
    TRY(ks_verify_sums(c, n, dl, bm));
    c->ksr.stat[3] += n; c->ksr.stat[4] += P.rep.size(); ++c->ksr.stat[5];
    return 0;
  }
  size_t checked = 0;
  enum : uint8_t { PASSED = 3, FAILED = 4 };                 // what a checked chunk's state byte becomes on the host
  {
    w.h_cstart.resize(M); w.h_clen.resize(M);
    for (size_t ch = 0; ch < M; ++ch) { w.h_cstart[ch] = P.chunks[ch].start; w.h_clen[ch] = P.chunks[ch].len; }
    TRY(upload(c, w.pos, P.pos.data(), 4 * n)); TRY(upload(c, w.order, P.order.data(), 4 * n)); TRY(upload(c, w.multi, P.multi.data(), n));
    TRY(upload(c, w.cstart, w.h_cstart.data(), 4 * M)); TRY(upload(c, w.clen, w.h_clen.data(), 4 * M));
    HIPCHK(c, w.elig.reserve(n)); HIPCHK(c, w.wt.reserve(8 * n)); HIPCHK(c, w.a.reserve(27 * 4 * n)); HIPCHK(c, w.b.reserve(54 * 4 * n));
    HIPCHK(c, w.ones.reserve(n)); HIPCHK(c, w.sa.reserve(27 * 4 * M)); HIPCHK(c, w.sb.reserve(54 * 4 * M)); HIPCHK(c, w.sb_ok.reserve(M));
    HIPCHK(c, w.cnt.reserve(4 * M)); HIPCHK(c, w.state.reserve(M)); HIPCHK(c, w.sa_bytes.reserve(64 * M));
    HIPCHK(c, hipMemsetAsync(w.ones.p, 1, n, c->stream));             // a weighted point is always a point: the flags of k_g2_seg_sum are not used
    TRY(seg_stage(c, w.seg, P.items_max, 54, true));
    if (com) {
      w.h_rowoff.resize(n);
      for (size_t g = 0; g < n; ++g) w.h_rowoff[g] = sel_off[g] - sel_off[0];
      TRY(upload(c, w.com, com, 4 * n)); TRY(upload(c, w.row_off, w.h_rowoff.data(), 8 * n));
      TRY(launch(c, c->stream, "ksr_elig", grid_lanes(n), k_ksr_elig, (const uint8_t*)c->kcom.sel.p, (const uint64_t*)w.row_off.p, (uint32_t)k->n, (const uint32_t*)w.com.p,
                 (const uint4*)k->cm.coms.p, (const uint32_t*)k->cm.cskip.p, (const uint32_t*)k->cm.cvalid.p, (const int32_t*)c->gs.sum.p, (const uint8_t*)c->gs.sum_ok.p, n,
                 d_sigs, (const uint8_t*)w.seed.p, (const uint8_t*)w.multi.p, (uint8_t*)w.elig.p, (uint64_t*)w.wt.p));
    } else {
      TRY(launch(c, c->stream, "ksr_elig", grid_lanes(n), k_ksr_elig, (const uint8_t*)c->kset.sel.p, (const uint64_t*)nullptr, (uint32_t)k->n, (const uint32_t*)nullptr,
                 (const uint4*)nullptr, (const uint32_t*)k->skip.p, (const uint32_t*)k->vwords.p, (const int32_t*)c->gs.sum.p, (const uint8_t*)c->gs.sum_ok.p, n, d_sigs,
                 (const uint8_t*)w.seed.p, (const uint8_t*)w.multi.p, (uint8_t*)w.elig.p, (uint64_t*)w.wt.p));
    }
    // A lane per group fills a fraction of the device and runs at the latency of its 64 steps: the G1 weights run on the second
    // stream BESIDE the G2 weights, which take three times as long
    HIPCHK(c, fork_stream2(c));
    TRY(launch(c, c->stream2, "ksr_weigh_g1", grid_lanes(n), k_ksr_weigh_g1, d_sigs, (const uint8_t*)w.elig.p, (const uint64_t*)w.wt.p, (const uint32_t*)w.pos.p, n,
               (int32_t*)w.a.p));
    HIPCHK(c, hipEventRecord(c->ev_join, c->stream2));
    TRY(launch(c, c->stream, "ksr_weigh_g2", grid_lanes(n), k_ksr_weigh_g2, (const int32_t*)c->gs.sum.p, (const uint8_t*)w.elig.p, (const uint64_t*)w.wt.p,
               (const uint32_t*)w.pos.p, n, (int32_t*)w.b.p));
    // the chunks' sums: the same runs for both sides, one after the other on the main stream (they share the ping-pong buffers)
    TRY(seg_run_levels(w.seg, P.levels, {(const int32_t*)w.b.p, n, (const uint8_t*)w.ones.p}, {(int32_t*)w.sb.p, M, (uint8_t*)w.sb_ok.p},
                       [&](SegSrc in, const uint32_t* start, const uint32_t* len, size_t runs, SegDst out, bool) {
      return launch(c, c->stream, "g2_seg_sum", grid_lanes(runs), k_g2_seg_sum, in.v, in.stride, in.ok, start, len, runs, out.v, out.stride, out.ok);
    }));
    HIPCHK(c, join_stream2(c));
    TRY(seg_run_levels(w.seg, P.levels, {(const int32_t*)w.a.p, n, nullptr}, {(int32_t*)w.sa.p, M, nullptr},
                       [&](SegSrc in, const uint32_t* start, const uint32_t* len, size_t runs, SegDst out, bool) {
      return launch(c, c->stream, "g1_seg_sum", grid_lanes(runs), k_g1_seg_sum, in.v, in.stride, (const uint32_t*)nullptr, start, len, runs, out.v, out.stride);
    }));
    TRY(launch(c, c->stream, "ksr_chunks", grid_lanes(M), k_ksr_chunks, (const int32_t*)w.sa.p, (const int32_t*)w.sb.p, M, (const uint32_t*)w.cstart.p,
               (const uint32_t*)w.clen.p, (const uint32_t*)w.order.p, (const uint8_t*)w.elig.p, (uint32_t*)w.cnt.p, (uint8_t*)w.state.p, (uint8_t*)w.sa_bytes.p));
    w.h_elig.resize(n); w.h_state.resize(M);
    HIPCHK(c, hipMemcpyAsync(w.h_elig.data(), w.elig.p, n, hipMemcpyDeviceToHost, c->stream));
    TRY(download(c, w.h_state.data(), w.state.p, M));
    // the chunks worth checking, as virtual tuples (sum B, the class's message, sum A)
    w.h_list.clear(); w.h_msgs.clear(); w.h_moff.assign(1, 0);
    for (size_t ch = 0; ch < M; ++ch)
      if (w.h_state[ch] == KSR_CHECK) { w.h_list.push_back((uint32_t)ch); ksr_push_msg(w, msgs, off, P.rep[P.chunks[ch].cls]); }
    checked = w.h_list.size();
    if (checked) {
      w.h_msgs.push_back(0);
      TRY(ksr_subcall(c, (const int32_t*)w.sb.p, M, nullptr, (const uint8_t*)w.sa_bytes.p, 0, dl));
      for (size_t j = 0; j < checked; ++j) w.h_state[w.h_list[j]] = bit_at(w.h_bits.data(), j) ? PASSED : FAILED;
    }
  }
  // every group's fate, in the caller's order
  std::memset(bm, 0, (n + 7) / 8);
  size_t decided = 0, failed = 0, direct = 0;
  w.h_list.clear(); w.h_msgs.clear(); w.h_moff.assign(1, 0);
  for (size_t g = 0; g < n; ++g) {
    const uint8_t st = w.h_state[P.chunk_of[g]];
    const bool e = w.h_elig[g] != 0;
    if (st == PASSED && e) { set_bit(bm, g); ++decided; continue; }
    if (st == FAILED && e) ++failed; else ++direct;
    w.h_list.push_back((uint32_t)g); ksr_push_msg(w, msgs, off, g);
  }
  // ... and everything the chunks did not decide: the exact pipeline on the gathered sums, one sub-call
  if (!w.h_list.empty()) {
    w.h_msgs.push_back(0);
    TRY(ksr_subcall(c, (const int32_t*)c->gs.sum.p, n, (const uint8_t*)c->gs.sum_ok.p, d_sigs, 1, dl));
    for (size_t j = 0; j < w.h_list.size(); ++j)
      if (bit_at(w.h_bits.data(), j)) set_bit(bm, w.h_list[j]);
  } else HIPCHK(c, hipStreamSynchronize(c->stream));
  c->ksr.stat[0] += decided; c->ksr.stat[1] += checked; c->ksr.stat[2] += failed; c->ksr.stat[3] += direct; c->ksr.stat[4] += P.rep.size(); ++c->ksr.stat[5];
  return 0;
}
// the arguments about messages that the host reads here (the exact calls leave them to the staging copy)
static int ksr_msg_args(const uint8_t* msgs, const uint64_t* off, size_t n) {
  if (check_offsets(off, n)) return BLSBN254_E_ARG;
  return (!msgs && off[n] != off[0]) ? BLSBN254_E_ARG : 0;
}

int blsbn254_keyset_fast_aggregate_verify_batch_rlc(blsbn254_ctx* c, const blsbn254_keyset* k, const uint8_t* sel, const uint8_t* msgs, const uint64_t* off,
                                                    const uint8_t* sigs, size_t n_groups, const uint8_t* dst, size_t dst_len, const uint8_t seed[32],
                                                    uint8_t* valid_bitmap) {
  if (!c || !k || k->ctx != c || !off || (n_groups && (!sel || !sigs || !valid_bitmap)) || (dst_len && !dst)) return BLSBN254_E_ARG;
  if (n_groups == 0) return 0;
  TRY(ks_args(c, k, sel, n_groups));
  TRY(ksr_msg_args(msgs, off, n_groups));
  ENTER(c);
  uint32_t dl;
  TRY(stage_dst(c, dst, dst_len, &dl));
  TRY(ksr_stage(c, sigs, seed, n_groups));
  size_t launches;
  TRY(ks_enqueue_sums(c, k, sel, n_groups, &launches));
  TRY(ksr_run(c, k, nullptr, nullptr, msgs, off, n_groups, dl, valid_bitmap));
  ks_tally(c, n_groups, launches);
  return 0;
}

int blsbn254_keyset_committee_fast_aggregate_verify_batch_rlc(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* com, const uint8_t* sel,
                                                              const uint64_t* sel_off, const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs, size_t n_groups,
                                                              const uint8_t* dst, size_t dst_len, const uint8_t seed[32], uint8_t* valid_bitmap) {
  if (!c || !k || k->ctx != c || !off || (n_groups && (!com || !sel || !sel_off || !sigs || !valid_bitmap)) || (dst_len && !dst)) return BLSBN254_E_ARG;
  if (n_groups == 0) return 0;
  TRY(kc_args(c, k, com, sel, sel_off, n_groups));
  TRY(ksr_msg_args(msgs, off, n_groups));
  ENTER(c);
  uint32_t dl;
  TRY(stage_dst(c, dst, dst_len, &dl));
  TRY(ksr_stage(c, sigs, seed, n_groups));
  TRY(kc_enqueue_call(c, k, com, sel, sel_off, n_groups));
  TRY(ksr_run(c, k, com, sel_off, msgs, off, n_groups, dl, valid_bitmap));
  kc_tally(c, n_groups);
  return 0;
}

int blsbn254_set_keyset_rlc_group(blsbn254_ctx* c, size_t group) {
  if (!c || (group && (group < KSR_MIN_GROUP || group > KSR_MAX_GROUP))) return BLSBN254_E_ARG;
  c->ksr_group = group ? group : KSR_DEFAULT_GROUP;
  return 0;
}
int blsbn254_keyset_rlc_stats(blsbn254_ctx* c, uint64_t out[6]) { return COPY_STATS(c, ksr.stat, 6, out); }

}  // extern "C"
