// host_keyset_committee.hip -- committees over a registered key set: index lists registered once ON the handle
// (blsbn254_keyset_set_committees) and the three read-side calls over RAGGED groups, each of which names a committee and brings a
// row as wide as that committee: sums, FastAggregateVerify and stake weights.  Every result is what the full-width call of
// host_keyset.hip / host_keyset_weight.hip gives on the row scattered over the registry.  Host side of include/blsbn254.h; kernels
// in k_keyset_committee.hip, lane functions in keyset_committee.h, the checks and the plan in keyset_committee_plan.h; see
// host_common.h and DESIGN.md 6l.
//
// A call's sums: the plan (kc_plan) sorts the groups by committee, cuts them into launches and items; per launch k_kc_count,
// k_kc_word_sum (a wave per item) and the segmented reduction of the group-major partials by the plan and runner of DESIGN.md 4b
// (plan_seg_levels, seg_run_levels with k_g2_seg_sum) into one point per sorted group; then ONE k_kc_finish for the call applies
// the complement against the committee's total and stores into the caller's order.  The totals of a table are what the same
// path gives for one all-ones row per committee with the flip forced off, before k_kc_finish.
#include "host_common.h"

extern "C" {

// The reduced sums U_i of every sorted group of c->kcom.plan (rows on the device at d_rows) into fin (column i = sorted position i;
// enqueued), the flip / ok bytes by sorted position into c->kcom.flip / ok.  noflip: every group is summed directly.
static int kc_enqueue_sums(blsbn254_ctx* c, const blsbn254_keyset* k, const uint8_t* d_rows, size_t n_groups, bool noflip, SegDst fin) {
  KcWs& w = c->kcom;
  const KcPlan& P = w.plan;
  HIPCHK(c, w.flip.reserve(n_groups)); HIPCHK(c, w.ok.reserve(n_groups));
  HIPCHK(c, w.part.reserve(54 * 4 * P.partials_max)); HIPCHK(c, w.part_ok.reserve(P.partials_max));
  HIPCHK(c, hipMemsetAsync(w.part_ok.p, 1, P.partials_max, c->stream));        // a word partial is always a point: the flags of k_g2_seg_sum are not used
  TRY(upload(c, w.scom, P.scom.data(), 4 * n_groups)); TRY(upload(c, w.srow, P.srow.data(), 8 * n_groups));
  TRY(upload(c, w.spbase, P.spbase.data(), 4 * n_groups)); TRY(upload(c, w.order, P.order.data(), 4 * n_groups));
  TRY(upload(c, w.items, P.items.data(), sizeof(KcItem) * P.items.size()));
  TRY(seg_stage(c, w.seg, P.items_max, 54, true));
  const uint4* coms = (const uint4*)k->cm.coms.p;
  for (const KcLaunch& L : P.launches) {
    const size_t m = L.hi - L.lo;
    TRY(launch(c, c->stream, "kc_count", grid_lanes(m), k_kc_count, d_rows, (const uint64_t*)w.srow.p, (const uint32_t*)w.scom.p, coms, (const uint32_t*)k->cm.cbad.p,
               L.lo, m, noflip ? 1 : 0, (uint8_t*)w.flip.p, (uint8_t*)w.ok.p));
    TRY(launch(c, c->stream, "kc_word_sum", Shape{dim3((unsigned)L.n_items), dim3(64)}, k_kc_word_sum, (const int32_t*)k->aff.p, (uint32_t)k->n,
               (const uint32_t*)k->cm.members.p, coms, (const uint32_t*)k->cm.cskip.p, (const uint4*)w.items.p + L.item0, d_rows, (const uint64_t*)w.srow.p,
               (const uint32_t*)w.scom.p, (const uint32_t*)w.spbase.p, (const uint8_t*)w.flip.p, (int32_t*)w.part.p, L.partials));
    TRY(seg_run_levels(w.seg, L.levels, {(const int32_t*)w.part.p, L.partials, (const uint8_t*)w.part_ok.p}, {fin.v + L.lo, fin.stride, fin.ok + L.lo},
                       [&](SegSrc in, const uint32_t* start, const uint32_t* len, size_t runs, SegDst out, bool) {
      return launch(c, c->stream, "g2_seg_sum", grid_lanes(runs), k_g2_seg_sum, in.v, in.stride, in.ok, start, len, runs, out.v, out.stride, out.ok);
    }));
  }
  return 0;
}

int blsbn254_keyset_set_committees(blsbn254_ctx* c, blsbn254_keyset* k, const uint32_t* members, const uint64_t* com_off, size_t n_com) {
  if (!c || !k || k->ctx != c || !members || !com_off) return BLSBN254_E_ARG;
  KcDev nw;                                                // the new table; after the swap below, the old one.  Freed on the way out,
  struct Settle { blsbn254_ctx* c; ~Settle() { (void)hipStreamSynchronize(c->stream); } } settle{c};   // ... behind everything enqueued
  if (!kc_build_table(members, com_off, n_com, k->n, nw.tab, c->last_error)) return BLSBN254_E_ARG;
  ENTER(c);
  KcWs& w = c->kcom;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  {                                                        // T names the new table only up to the swap below
  const KcTable& T = nw.tab;
  TRY(upload(c, nw.members, members, 4 * T.members));
  TRY(upload(c, nw.coms, T.com.data(), sizeof(KcCom) * n_com));
  TRY(upload(c, w.wcom, T.wcom.data(), 4 * T.words));
  HIPCHK(c, nw.cbad.reserve(4 * T.words)); HIPCHK(c, nw.cskip.reserve(4 * T.words)); HIPCHK(c, nw.cvalid.reserve(4 * T.words));
  HIPCHK(c, nw.totals.reserve(54 * 4 * n_com));
  TRY(launch(c, c->stream, "kc_words", grid_lanes(T.words), k_kc_words, (const uint32_t*)nw.members.p, (const uint4*)nw.coms.p, (const uint32_t*)w.wcom.p, T.words,
             (const uint32_t*)k->bad.p, (const uint32_t*)k->skip.p, (const uint32_t*)k->vwords.p, (uint32_t*)nw.cbad.p, (uint32_t*)nw.cskip.p, (uint32_t*)nw.cvalid.p));
  // the totals: the call's own sum path on one all-ones row per committee, summed directly (ctx-owned arrays: they outlive the uploads)
  w.h_off.assign(1, 0); w.h_com.resize(n_com); w.h_ones.clear();
  for (size_t i = 0; i < n_com; ++i) {
    const uint32_t size = T.com[i].size, rb = kc_row_bytes(size);
    w.h_ones.insert(w.h_ones.end(), rb, 0xff);
    if (size & 7) w.h_ones.back() = (uint8_t)(0xffu >> (8 - (size & 7)));
    w.h_off.push_back(w.h_ones.size());
    w.h_com[i] = (uint32_t)i;
  }
  if (!kc_plan(T, w.h_com.data(), w.h_off.data(), n_com, c->chunk, w.plan, w.seg.h_start, w.seg.h_len)) { c->last_error = "internal: committee sums do not converge"; return BLSBN254_E_HIP; }
  TRY(upload(c, w.sel, w.h_ones.data(), w.h_ones.size()));
  HIPCHK(c, w.u_ok.reserve(n_com));
  }
  k->cm.swap(nw);                                          // from here on nw holds the OLD table
  int rc = kc_enqueue_sums(c, k, (const uint8_t*)w.sel.p, n_com, true, {(int32_t*)k->cm.totals.p, n_com, (uint8_t*)w.u_ok.p});
  if (!rc) { hipError_t e = hipStreamSynchronize(c->stream); if (e != hipSuccess) { c->last_error = std::string("hipStreamSynchronize: ") + hipGetErrorString(e); rc = BLSBN254_E_HIP; } }
  if (rc) { (void)hipStreamSynchronize(c->stream); k->cm.swap(nw); return rc; }     // the handle keeps the table it had
  ++c->kcom.stat[3];
  return 0;
}

size_t blsbn254_keyset_committee_count(const blsbn254_keyset* k) { return k ? k->cm.tab.com.size() : 0; }

// the checks the three calls share (n_groups > 0)
int kc_args(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* com, const uint8_t* sel, const uint64_t* sel_off, size_t n_groups) {
  if (k->cm.tab.com.empty()) { c->last_error = "the key set has no committees (blsbn254_keyset_set_committees)"; return BLSBN254_E_ARG; }
  if (n_groups > c->chunk) { c->last_error = "more groups than one launch chunk"; return BLSBN254_E_ARG; }
  return kc_check_rows(k->cm.tab, com, sel, sel_off, n_groups, c->last_error) ? 0 : BLSBN254_E_ARG;
}
// the call's rows staged (uploaded to c->kcom.sel), its plan made, its sums into c->gs.sum / c->gs.sum_ok in the caller's order (enqueued); the flip bytes
// into c->kcom.h_flip (enqueued: read after the caller's synchronising download)
int kc_enqueue_call(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* com, const uint8_t* sel, const uint64_t* sel_off, size_t n_groups) {
  KcWs& w = c->kcom;
  TRY(upload(c, w.sel, sel + sel_off[0], sel_off[n_groups] - sel_off[0]));
  return kc_enqueue_call_dev(c, k, com, (const uint8_t*)w.sel.p, sel_off, n_groups);
}
// the same behind the upload, for a caller whose rows are on the device already (host_keyset_committee_agg.hip)
int kc_enqueue_call_dev(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* com, const uint8_t* d_rows, const uint64_t* sel_off, size_t n_groups) {
  KcWs& w = c->kcom;
  if (!kc_plan(k->cm.tab, com, sel_off, n_groups, c->chunk, w.plan, w.seg.h_start, w.seg.h_len)) { c->last_error = "internal: committee sums do not converge"; return BLSBN254_E_HIP; }
  HIPCHK(c, w.u.reserve(54 * 4 * n_groups)); HIPCHK(c, w.u_ok.reserve(n_groups));
  HIPCHK(c, c->gs.sum.reserve(n_groups * 54 * 4)); HIPCHK(c, c->gs.sum_ok.reserve(n_groups));
  TRY(kc_enqueue_sums(c, k, d_rows, n_groups, false, {(int32_t*)w.u.p, n_groups, (uint8_t*)w.u_ok.p}));
  TRY(launch(c, c->stream, "kc_finish", grid_lanes(n_groups), k_kc_finish, (const int32_t*)w.u.p, n_groups, n_groups, (const uint32_t*)w.scom.p, (const uint32_t*)w.order.p,
             (const int32_t*)k->cm.totals.p, k->cm.tab.com.size(), (const uint8_t*)w.flip.p, (const uint8_t*)w.ok.p, (int32_t*)c->gs.sum.p, n_groups, (uint8_t*)c->gs.sum_ok.p));
  w.h_flip.resize(n_groups);
  HIPCHK(c, hipMemcpyAsync(w.h_flip.data(), w.flip.p, n_groups, hipMemcpyDeviceToHost, c->stream));
  return 0;
}
// counted once the call has succeeded (and synchronised: the flip bytes are on the host)
void kc_tally(blsbn254_ctx* c, size_t n_groups) {
  c->kcom.stat[0] += n_groups; c->kcom.stat[2] += c->kcom.plan.launches.size();
  for (size_t i = 0; i < n_groups; ++i) c->kcom.stat[1] += c->kcom.h_flip[i] ? 1 : 0;
}

int blsbn254_keyset_committee_sum_batch(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* com, const uint8_t* sel, const uint64_t* sel_off, size_t n_groups,
                                        uint8_t* out, uint8_t* status) {
  if (!c || !k || k->ctx != c || (n_groups && (!com || !sel || !sel_off || !out || !status))) return BLSBN254_E_ARG;
  if (n_groups == 0) return 0;
  TRY(kc_args(c, k, com, sel, sel_off, n_groups));
  ENTER(c);
  TRY(kc_enqueue_call(c, k, com, sel, sel_off, n_groups));
  HIPCHK(c, c->out.reserve(128 * n_groups));
  TRY(launch(c, c->stream, "g2p_to_bytes", grid_lanes(n_groups), k_g2p_to_bytes, (const int32_t*)c->gs.sum.p, n_groups, (const uint8_t*)c->gs.sum_ok.p, n_groups,
             (uint8_t*)c->out.p, 0));
  HIPCHK(c, hipMemcpyAsync(out, c->out.p, 128 * n_groups, hipMemcpyDeviceToHost, c->stream));
  TRY(download(c, status, c->gs.sum_ok.p, n_groups));
  kc_tally(c, n_groups);
  return 0;
}

// both forms of the entry point; compressed: sigs holds 32 bytes per group (stage_g1)
static int kc_verify(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* com, const uint8_t* sel, const uint64_t* sel_off, const uint8_t* msgs,
                     const uint64_t* off, const uint8_t* sigs, size_t n_groups, const uint8_t* dst, size_t dst_len, uint8_t* valid_bitmap, bool compressed) {
  if (!c || !k || k->ctx != c || !off || (n_groups && (!com || !sel || !sel_off || !sigs || !valid_bitmap)) || (dst_len && !dst)) return BLSBN254_E_ARG;
  if (n_groups == 0) return 0;
  TRY(kc_args(c, k, com, sel, sel_off, n_groups));
  ENTER(c);
  uint32_t dl;
  TRY(stage_dst(c, dst, dst_len, &dl));
  TRY(stage_msgs(c, msgs, off, n_groups));
  HIPCHK(c, c->gs.pk.reserve(128 * n_groups)); HIPCHK(c, c->bitmap.reserve((n_groups + 7) / 8 + 8));
  TRY(stage_g1(c, sigs, n_groups, compressed));
  TRY(kc_enqueue_call(c, k, com, sel, sel_off, n_groups));
  TRY(ks_verify_sums(c, n_groups, dl, valid_bitmap));
  kc_tally(c, n_groups);
  return 0;
}
int blsbn254_keyset_committee_fast_aggregate_verify_batch(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* com, const uint8_t* sel, const uint64_t* sel_off,
                                                          const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs, size_t n_groups, const uint8_t* dst,
                                                          size_t dst_len, uint8_t* valid_bitmap) {
  return kc_verify(c, k, com, sel, sel_off, msgs, off, sigs, n_groups, dst, dst_len, valid_bitmap, false);
}
int blsbn254_keyset_committee_fast_aggregate_verify_batch_compressed(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* com, const uint8_t* sel,
                                                                     const uint64_t* sel_off, const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs,
                                                                     size_t n_groups, const uint8_t* dst, size_t dst_len, uint8_t* valid_bitmap) {
  return kc_verify(c, k, com, sel, sel_off, msgs, off, sigs, n_groups, dst, dst_len, valid_bitmap, true);
}

int blsbn254_keyset_committee_weight_batch(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* com, const uint8_t* sel, const uint64_t* sel_off, size_t n_groups,
                                           uint64_t* out) {
  if (!c || !k || k->ctx != c || (n_groups && (!com || !sel || !sel_off || !out))) return BLSBN254_E_ARG;
  if (k->n_cols == 0) { c->last_error = "the key set has no weights (blsbn254_keyset_set_weights)"; return BLSBN254_E_ARG; }
  if (n_groups == 0) return 0;
  TRY(kc_args(c, k, com, sel, sel_off, n_groups));
  ENTER(c);
  KcWs& w = c->kcom;
  // the groups stay in the caller's order: a wave per group needs no neighbours (ctx-owned offsets: they outlive the upload)
  w.h_off.resize(n_groups);
  for (size_t g = 0; g < n_groups; ++g) w.h_off[g] = sel_off[g] - sel_off[0];
  HIPCHK(c, w.wout.reserve(8 * k->n_cols * n_groups));
  TRY(upload(c, w.sel, sel + sel_off[0], sel_off[n_groups] - sel_off[0]));
  TRY(upload(c, w.srow, w.h_off.data(), 8 * n_groups)); TRY(upload(c, w.scom, com, 4 * n_groups));
  const size_t Gl = kw_launch_groups(c->chunk);
  for (size_t lo = 0; lo < n_groups; lo += Gl) {
    const size_t m = std::min(Gl, n_groups - lo);
    TRY(launch(c, c->stream, "kc_weight", grid_lanes(64 * m), k_kc_weight, (const uint8_t*)w.sel.p, (const uint64_t*)w.srow.p, (const uint32_t*)w.scom.p,
               (const uint4*)k->cm.coms.p, (const uint32_t*)k->cm.members.p, (const uint32_t*)k->cm.cvalid.p, (const uint64_t*)k->weff.p, (uint32_t)k->n_cols, lo, m,
               (uint64_t*)w.wout.p));
  }
  TRY(download(c, out, w.wout.p, 8 * k->n_cols * n_groups));
  c->kcom.stat[0] += n_groups;
  return 0;
}

int blsbn254_keyset_committee_stats(blsbn254_ctx* c, uint64_t out[4]) { return COPY_STATS(c, kcom.stat, 4, out); }

}  // extern "C"
