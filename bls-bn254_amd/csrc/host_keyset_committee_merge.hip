// host_keyset_committee_merge.hip -- checked merge of partial aggregates PER COMMITTEE of a registered key set:
// host_keyset_merge.hip for the intermediate node whose partial aggregates arrive per committee.  A group names a committee of
// the handle's table and brings contributions (a row as wide as the COMMITTEE, an aggregate signature); out come one merged
// aggregate and one merged row as wide as the committee, which the read-side committee calls of host_keyset_committee.hip
// consume as they are.  Nothing is as wide as the registry.  Host side of include/blsbn254.h; the kernel in
// k_keyset_committee_merge.hip, lane functions in keyset_committee_merge.h, the argument walk, the ragged layout and the repack
// in keyset_committee_merge_plan.h; see host_common.h and DESIGN.md 6p.
//
// The two attempts are those of host_keyset_merge.hip, each ONE pass of enqueued work and one download:
//   optimistic   the signature test of every contribution and its signature as a point (k_km_sig), the greedy selection of
//                disjoint candidates in the order given, a wave per group over the group's ragged rows, which leaves the merged
//                rows at their sel_off positions (k_kcm_select), the identity over the points of what was not selected and the
//                used / candidate bitmaps (k_km_points), the signature sums (k_g1_seg_sum by levels, k_g1p_to_bytes), the key
//                sums from the merged rows ON THE DEVICE by the committee path (kc_enqueue_call_dev), and ONE verification per
//                group of (key sum, message, signature sum).
//   fallback     only for groups that selected something and failed, EVERY candidate of theirs repacked by the host into a
//                sub-call: each contribution verified on its own as a one-row group of the committee path
//                (kc_enqueue_call_dev over the contribution rows where the sub-call's rows already are on the device, the
//                group's message once per contribution), then the SAME pass with those bits as the selection's mask.  No failing
//                group: nothing is launched.
// A group's outcome depends on its own inputs only: which attempt served it, where a launch ended and how many groups shared
// the call do not change a byte.
//
// The wire-format form (blsbn254_keyset_committee_merge_checked_batch_compressed) shares this body behind
// KcmCall::wire exactly as host_keyset_merge.hip does: 32-byte signatures uploaded to w.wire and inflated into w.sigs, the sums
// out in both encodings (k_g1p_to_wire), 32-byte signatures in the fallback's repack.
#include "host_common.h"

extern "C" {

static const size_t KCM_SUM_GROUP = 16;                      // signatures per lane and level of the group sums
static const uint64_t KCM_MAX_ROW_BYTES = (uint64_t)1 << 30; // contribution rows of one call, together

namespace {
struct KcmCall {
  const uint32_t* com; const uint8_t* rows; const uint64_t* row_off;      // rows / sigs / msgs indexed by the offsets as given
  const uint8_t* sigs; const uint64_t* con_off;
  const uint8_t* msgs; const uint64_t* msg_off; const uint64_t* sel_off;
  size_t n_groups;
  const uint8_t* dst; size_t dst_len;
  bool wire;                                                           // sigs holds 32 bytes per contribution, the sums leave compressed too
};
}

// One attempt over the groups of A, enqueued: the signature sums' encodings into c->kcmrg.out, the merged rows into c->kcmrg.urows
// (row g at sel_off[g] - sel_off[0]), the used / candidate bitmaps into c->kcmrg.used / cand, the bits of the groups' equation
// into c->kcmrg.gbits; A.wire: the sums' compressed encodings into c->kcmrg.wout as well.
static int kcm_attempt(blsbn254_ctx* c, const blsbn254_keyset* k, const KcmCall& A, bool fallback) {
  KcmWs& w = c->kcmrg;
  const size_t ng = A.n_groups;
  TRY(stage_group_offsets(c, w.goff, A.con_off, ng));
  const size_t N = w.goff.h[ng], N1 = N ? N : 1, nb = (N + 7) / 8;
  kcm_layout(A.row_off, A.sel_off, ng, w.h_rbase, w.h_roff);              // (ctx-owned: the arrays outlive the uploads)
  const size_t in_bytes = w.h_rbase[ng], out_bytes = w.h_roff[ng];
  TRY(upload(c, w.com, A.com, 4 * ng));
  TRY(upload(c, w.rbase, w.h_rbase.data(), 8 * (ng + 1))); TRY(upload(c, w.roff, w.h_roff.data(), 8 * (ng + 1)));
  HIPCHK(c, w.rows.reserve(in_bytes ? in_bytes : 1)); HIPCHK(c, w.sigs.reserve(64 * N1));
  if (N) {
    TRY(upload(c, w.rows, A.rows + A.row_off[0], in_bytes));
    if (!A.wire) TRY(upload(c, w.sigs, A.sigs + 64 * A.con_off[0], 64 * N));
    else {
      TRY(upload(c, w.wire, A.sigs + 32 * A.con_off[0], 32 * N));
      TRY(g1_inflate_dev(c, (const uint8_t*)w.wire.p, N, (uint8_t*)w.sigs.p));
    }
  }
  const size_t n_pk = fallback ? std::max(std::min(N, c->chunk), ng) : ng;
  HIPCHK(c, c->gs_pk.reserve(128 * n_pk)); HIPCHK(c, c->gs_sum.reserve(n_pk * 54 * 4)); HIPCHK(c, c->gs_sum_ok.reserve(n_pk));
  uint32_t dl;
  TRY(stage_dst(c, A.dst, A.dst_len, &dl));
  if (fallback && N) {
    // every contribution as the tuple (the key sum of its row, the group's message, its signature): a contribution is a one-row
    // group of its group's committee, the group's message once per contribution (ctx-owned: outlives the upload), by launches
    // of at most c->chunk contributions, the bits into w.vbits.  The plan of a launch lives in c->kcom and the next launch (or
    // the groups' equation below) plans over it: a launch is settled before the next one is planned
    HIPCHK(c, w.vbits.reserve(nb + 8));
    kcm_layout_contributions(k->cm.tab, A.com, A.con_off, ng, w.h_ccom, w.h_coff);
    w.s_emsgs.clear(); w.s_emoff.assign(1, 0);
    for (size_t g = 0; g < ng; ++g)
      for (uint32_t s = w.goff.h[g]; s < w.goff.h[g + 1]; ++s) {
        if (A.msg_off[g + 1] != A.msg_off[g]) w.s_emsgs.insert(w.s_emsgs.end(), A.msgs + A.msg_off[g], A.msgs + A.msg_off[g + 1]);
        w.s_emoff.push_back(w.s_emsgs.size());
      }
    TRY(for_chunks(c, N, [&](size_t lo, size_t m) {
      TRY(kc_enqueue_call_dev(c, k, w.h_ccom.data() + lo, (const uint8_t*)w.rows.p + w.h_coff[lo], w.h_coff.data() + lo, m));
      TRY(launch(c, c->stream, "g2p_to_bytes", grid_lanes(m), k_g2p_to_bytes, (const int32_t*)c->gs_sum.p, m, (const uint8_t*)c->gs_sum_ok.p, m, (uint8_t*)c->gs_pk.p, 1));
      TRY(stage_msgs(c, w.s_emsgs.data(), w.s_emoff.data() + lo, m));
      TRY(verify_chunk_dev(c, (const uint8_t*)c->gs_pk.p, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, (const uint8_t*)w.sigs.p + 64 * lo, m, dl,
                           (uint8_t*)w.vbits.p + (lo >> 3)));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      return 0;
    }));
  }
  HIPCHK(c, w.sig_ok.reserve(N1)); HIPCHK(c, w.flags.reserve(N1)); HIPCHK(c, w.used.reserve(nb + 8)); HIPCHK(c, w.cand.reserve(nb + 8));
  HIPCHK(c, w.pts.reserve(27 * N1 * 4)); HIPCHK(c, w.urows.reserve(out_bytes ? out_bytes : 1));
  HIPCHK(c, w.gsum.reserve(27 * ng * 4)); HIPCHK(c, w.out.reserve(64 * ng)); HIPCHK(c, w.gbits.reserve((ng + 7) / 8 + 8));
  const uint32_t* goff = (const uint32_t*)w.goff.d.p;
  TRY(for_chunks(c, N, [&](size_t lo, size_t m) {
    return launch(c, c->stream, "km_sig", grid_lanes(m), k_km_sig, (const uint8_t*)w.sigs.p, m, (uint32_t)lo, N, (uint8_t*)w.sig_ok.p, (int32_t*)w.pts.p);
  }));
  // (the signature bytes are complete: every launch of the test is enqueued before the first group is walked)  A wave per group:
  // a launch of c->chunk lanes walks c->chunk / 64 groups
  const size_t Gl = std::max((size_t)1, c->chunk / 64);
  for (size_t lo = 0; lo < ng; lo += Gl) {
    const size_t m = std::min(Gl, ng - lo);
    TRY(launch(c, c->stream, "kcm_select", grid_lanes(64 * m), k_kcm_select, (const uint8_t*)w.rows.p, (const uint8_t*)w.sig_ok.p,
               fallback ? (const uint8_t*)w.vbits.p : (const uint8_t*)nullptr, goff, (const uint32_t*)w.com.p, (const uint4*)k->cm.coms.p,
               (const uint32_t*)k->cm.cvalid.p, (const uint64_t*)w.rbase.p, (const uint64_t*)w.roff.p, lo, m, (uint8_t*)w.flags.p, (uint8_t*)w.urows.p));
  }
  TRY(for_chunks(c, N, [&](size_t lo, size_t m) {
    return launch(c, c->stream, "km_points", grid_lanes(m), k_km_points, (const uint8_t*)w.flags.p, m, (uint32_t)lo, N, (int32_t*)w.pts.p, (uint8_t*)w.used.p,
                  (uint8_t*)w.cand.p);
  }));
  // the signature sums: launches of whole groups, planned up front
  w.seg.h_start.clear(); w.seg.h_len.clear();
  std::vector<SegLaunch> launches;
  size_t m_max, items_max;
  if (!plan_launches_whole(w.goff.h, ng, c->chunk, KCM_SUM_GROUP, (size_t)-1, launches, w.seg.h_start, w.seg.h_len, &m_max, &items_max)) {
    c->last_error = "internal: group sums do not converge";
    return BLSBN254_E_HIP;
  }
  TRY(seg_stage(c, w.seg, items_max, 27, false));
  for (const SegLaunch& L : launches)
    TRY(seg_run_levels(w.seg, L.levels, {(const int32_t*)w.pts.p + L.lo, N1, nullptr}, {(int32_t*)w.gsum.p + L.ga, ng, nullptr},
                       [&](SegSrc in, const uint32_t* start, const uint32_t* len, size_t runs, SegDst out, bool) {
      return launch(c, c->stream, "g1_seg_sum", grid_lanes(runs), k_g1_seg_sum, in.v, in.stride, (const uint32_t*)nullptr, start, len, runs, out.v, out.stride);
    }));
  if (A.wire) {
    HIPCHK(c, w.wout.reserve(32 * ng));
    TRY(launch(c, c->stream, "g1p_to_wire", grid_lanes(ng), k_g1p_to_wire, (const int32_t*)w.gsum.p, ng, ng, (uint8_t*)w.out.p, (uint8_t*)w.wout.p));
  } else TRY(launch(c, c->stream, "g1p_to_bytes", grid_lanes(ng), k_g1p_to_bytes, (const int32_t*)w.gsum.p, ng, ng, (uint8_t*)w.out.p));
  // the key sums from the merged rows where they are, by the committee path, then the equation of the committee verify
  TRY(kc_enqueue_call_dev(c, k, A.com, (const uint8_t*)w.urows.p, A.sel_off, ng));
  TRY(launch(c, c->stream, "g2p_to_bytes", grid_lanes(ng), k_g2p_to_bytes, (const int32_t*)c->gs_sum.p, ng, (const uint8_t*)c->gs_sum_ok.p, ng, (uint8_t*)c->gs_pk.p, 1));
  TRY(stage_msgs(c, A.msgs, A.msg_off, ng));               // ONE message per group
  return verify_chunk_dev(c, (const uint8_t*)c->gs_pk.p, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, (const uint8_t*)w.out.p, ng, dl, (uint8_t*)w.gbits.p);
}

static inline bool kcm_bit(const std::vector<uint8_t>& bm, size_t i) { return (bm[i >> 3] >> (i & 7)) & 1; }

// both forms of the entry point; wire: sigs and out_sigs hold 32 bytes per signature
static int kcm_checked(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* com, const uint8_t* rows, const uint64_t* row_off, const uint8_t* sigs,
                       const uint64_t* con_off, const uint8_t* msgs, const uint64_t* msg_off, const uint64_t* sel_off, size_t n_groups, const uint8_t* dst,
                       size_t dst_len, uint8_t* out_sigs, uint8_t* out_sel, uint8_t* used, uint8_t* status, bool wire) {
  if (!c) return BLSBN254_E_ARG;
  if (!k) { c->last_error = "a NULL argument"; return BLSBN254_E_ARG; }
  if (k->ctx != c) { c->last_error = "the key set belongs to another context"; return BLSBN254_E_ARG; }
  if (n_groups == 0) return 0;
  if (!com || !row_off || !con_off || !msg_off || !sel_off || !out_sigs || !out_sel || !used || !status || (dst_len && !dst)) {
    c->last_error = "a NULL argument";
    return BLSBN254_E_ARG;
  }
  if (k->cm.tab.com.empty()) { c->last_error = "the key set has no committees (blsbn254_keyset_set_committees)"; return BLSBN254_E_ARG; }
  if (n_groups > c->chunk) { c->last_error = "more groups than one launch chunk"; return BLSBN254_E_ARG; }
  if (check_offsets(con_off, n_groups)) { c->last_error = "contribution offsets decrease"; return BLSBN254_E_ARG; }
  if (check_offsets(msg_off, n_groups)) { c->last_error = "message offsets decrease"; return BLSBN254_E_ARG; }
  if (!msgs && msg_off[n_groups] != msg_off[0]) { c->last_error = "a NULL argument"; return BLSBN254_E_ARG; }
  if (con_off[n_groups] != con_off[0] && (!rows || !sigs)) { c->last_error = "a NULL argument"; return BLSBN254_E_ARG; }
  const KcTable& T = k->cm.tab;
  const KcmWalk wk = kcm_walk(T, com, rows, row_off, con_off, sel_off, n_groups, MAX_LANES, KCM_MAX_ROW_BYTES);
  if (wk.code != KCM_OK) {
    const std::string who = "group " + std::to_string(wk.group);
    c->last_error = wk.code == KCM_TOO_MANY ? "more than 2^23 contributions in one call"
                  : wk.code == KCM_ROWS_TOO_LARGE ? "more than 2^30 bytes of rows in one call"
                  : wk.code == KCM_COM_RANGE ? who + " names committee " + std::to_string(com[wk.group]) + " of " + std::to_string(T.com.size())
                  : wk.code == KCM_ROW_SPAN ? who + ": the contribution rows must be " + std::to_string(con_off[wk.group + 1] - con_off[wk.group]) + " x " +
                                              std::to_string(kc_row_bytes(T.com[com[wk.group]].size)) + " bytes"
                  : wk.code == KCM_SEL_LEN ? who + ": the row must be " + std::to_string(kc_row_bytes(T.com[com[wk.group]].size)) + " bytes"
                  : wk.code == KCM_ROW_PAD ? "contribution " + std::to_string(wk.con - con_off[0]) + " sets a bit past the last member"
                  : wk.which == 1 ? "contribution row offsets decrease" : wk.which == 2 ? "row offsets decrease" : "contribution offsets decrease";
    return BLSBN254_E_ARG;
  }
  ENTER(c);
  KcmWs& w = c->kcmrg;
  const size_t gb = (n_groups + 7) / 8, total = sel_off[n_groups] - sel_off[0], sb = wire ? 32 : 64;
  const size_t N = (size_t)(con_off[n_groups] - con_off[0]), nb = (N + 7) / 8;
  const DevBuf& d_out = wire ? w.wout : w.out;                         // the sums as the caller gets them
  const KcmCall A{com, rows, row_off, sigs, con_off, msgs, msg_off, sel_off, n_groups, dst, dst_len, wire};
  TRY(kcm_attempt(c, k, A, false));
  w.h_gbits.assign(gb, 0); w.h_used.assign(nb + 1, 0); w.h_cand.assign(nb + 1, 0);
  HIPCHK(c, hipMemcpyAsync(out_sigs, d_out.p, sb * n_groups, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(out_sel, w.urows.p, total, hipMemcpyDeviceToHost, c->stream));
  if (nb) {
    HIPCHK(c, hipMemcpyAsync(w.h_used.data(), w.used.p, nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(w.h_cand.data(), w.cand.p, nb, hipMemcpyDeviceToHost, c->stream));
  }
  TRY(download(c, w.h_gbits.data(), w.gbits.p, gb));
  // a group whose equation holds: its selected contributions are used.  One whose equation does not hold: the identity, a zero
  // row, no used bit -- and the fallback if its merged row shows that something was selected
  std::memset(used, 0, nb);
  w.fail.clear();
  for (size_t g = 0; g < n_groups; ++g) {
    if (kcm_bit(w.h_gbits, g)) {
      status[g] = 0; ++c->stat_kcmrg[0];
      for (uint64_t s = con_off[g] - con_off[0]; s < con_off[g + 1] - con_off[0]; ++s)
        if (kcm_bit(w.h_used, s)) used[s >> 3] |= (uint8_t)(1u << (s & 7));
      continue;
    }
    status[g] = BLSBN254_ST_SHORT;
    g1_identity_out(out_sigs + sb * g, wire);
    uint8_t *row = out_sel + (sel_off[g] - sel_off[0]), *end = out_sel + (sel_off[g + 1] - sel_off[0]);
    if (std::any_of(row, end, [](uint8_t b) { return b != 0; })) w.fail.push_back(g);
    else ++c->stat_kcmrg[3];
    std::memset(row, 0, end - row);
  }
  if (w.fail.empty()) return 0;
  // the sub-call over the failing groups' candidates, repacked (ctx-owned: the arrays outlive the asynchronous uploads)
  const size_t nf = w.fail.size();
  kcm_repack(T, w.fail, com, rows, row_off, sigs, con_off, w.h_cand.data(), w.sub, sb);
  const size_t Ns = w.sub.pos.size();
  w.s_msgs.clear(); w.s_moff.assign(1, 0);
  for (size_t g : w.fail) {
    if (msg_off[g + 1] != msg_off[g]) w.s_msgs.insert(w.s_msgs.end(), msgs + msg_off[g], msgs + msg_off[g + 1]);
    w.s_moff.push_back(w.s_msgs.size());
  }
  c->stat_kcmrg[1] += nf; c->stat_kcmrg[2] += Ns;
  const KcmCall B{w.sub.com.data(), w.sub.rows.data(), w.sub.row_off.data(), w.sub.sigs.data(), w.sub.off.data(), w.s_msgs.data(), w.s_moff.data(),
                  w.sub.sel_off.data(), nf, dst, dst_len, wire};
  TRY(kcm_attempt(c, k, B, true));
  const size_t nbs = (Ns + 7) / 8, sub_total = w.sub.sel_off[nf];
  w.s_out.resize(sb * nf); w.s_rows.resize(sub_total); w.h_gbits.assign((nf + 7) / 8, 0); w.h_used.assign(nbs + 1, 0);
  HIPCHK(c, hipMemcpyAsync(w.s_out.data(), d_out.p, sb * nf, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(w.s_rows.data(), w.urows.p, sub_total, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(w.h_used.data(), w.used.p, nbs, hipMemcpyDeviceToHost, c->stream));
  TRY(download(c, w.h_gbits.data(), w.gbits.p, (nf + 7) / 8));
  for (size_t j = 0; j < nf; ++j) {
    const size_t g = w.fail[j];
    if (!kcm_bit(w.h_gbits, j)) { ++c->stat_kcmrg[3]; continue; }
    status[g] = 0;
    std::memcpy(out_sigs + sb * g, w.s_out.data() + sb * j, sb);
    std::memcpy(out_sel + (sel_off[g] - sel_off[0]), w.s_rows.data() + w.sub.sel_off[j], sel_off[g + 1] - sel_off[g]);
    for (uint64_t i = w.sub.off[j]; i < w.sub.off[j + 1]; ++i)
      if (kcm_bit(w.h_used, i)) { const uint64_t s = w.sub.pos[i] - con_off[0]; used[s >> 3] |= (uint8_t)(1u << (s & 7)); }
  }
  return 0;
}

int blsbn254_keyset_committee_merge_checked_batch(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* com, const uint8_t* rows, const uint64_t* row_off,
                                                  const uint8_t* sigs, const uint64_t* con_off, const uint8_t* msgs, const uint64_t* msg_off, const uint64_t* sel_off,
                                                  size_t n_groups, const uint8_t* dst, size_t dst_len, uint8_t* out_sigs, uint8_t* out_sel, uint8_t* used,
                                                  uint8_t* status) {
  return kcm_checked(c, k, com, rows, row_off, sigs, con_off, msgs, msg_off, sel_off, n_groups, dst, dst_len, out_sigs, out_sel, used, status, false);
}
int blsbn254_keyset_committee_merge_checked_batch_compressed(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* com, const uint8_t* rows,
                                                             const uint64_t* row_off, const uint8_t* sigs, const uint64_t* con_off, const uint8_t* msgs,
                                                             const uint64_t* msg_off, const uint64_t* sel_off, size_t n_groups, const uint8_t* dst, size_t dst_len,
                                                             uint8_t* out_sigs, uint8_t* out_sel, uint8_t* used, uint8_t* status) {
  return kcm_checked(c, k, com, rows, row_off, sigs, con_off, msgs, msg_off, sel_off, n_groups, dst, dst_len, out_sigs, out_sel, used, status, true);
}

int blsbn254_keyset_committee_merge_stats(blsbn254_ctx* c, uint64_t out[4]) {
  if (!c || !out) return BLSBN254_E_ARG;
  for (int i = 0; i < 4; ++i) out[i] = c->stat_kcmrg[i];
  return 0;
}

}  // extern "C"
