// host_keyset_committee_agg.hip -- checked signature aggregation PER COMMITTEE of a registered key set: host_keyset_agg.hip for
// the collector whose signatures arrive per committee.  A group names a committee of the handle's table and brings entries
// (position in the member list, signature); out come the aggregate and a row as wide as the COMMITTEE, which the read-side
// committee calls of host_keyset_committee.hip consume as they are.  Nothing is as wide as the registry.  Host side of
// include/blsbn254.h; kernels in k_keyset_committee_agg.hip, lane functions in keyset_committee_agg.h, the argument walk, the
// ragged layout and the repack in keyset_committee_agg_plan.h; see host_common.h and DESIGN.md 6o.
//
// The two attempts are those of host_keyset_agg.hip, each ONE pass of enqueued work and one download:
//   optimistic   the candidate bit of every entry and its signature as a point (k_kca_scan: the validity bit of the entry's
//                position in the committee's words, no member index), the ragged rows from those bits (k_kca_rows), the signature
//                sums (k_g1_seg_sum by levels, k_g1p_to_bytes), the key sums from the rows ON THE DEVICE by the committee path
//                (kc_enqueue_call_dev), and ONE verification per group of (key sum, message, signature sum).
//   fallback     only for groups that had a candidate and failed, their candidates repacked by the host into a sub-call: every
//                entry's registry index resolved from the member list (k_kca_resolve), its key gathered by it (k_ka_gather_keys),
//                every signature verified on its own, then the SAME pass with those bits as the scan's mask.
// A group's outcome depends on its own inputs only.
//
// The wire-format form (blsbn254_keyset_committee_aggregate_checked_batch_compressed) shares this body behind
// KcaCall::wire exactly as host_keyset_agg.hip does: the optimistic attempt scans the 32-byte entries where they are uploaded
// (k_kca_scan_wire), the sums leave in both encodings (k_g1p_to_wire), the fallback inflates its repacked entries into w.sigs.
#include "host_common.h"

extern "C" {

static const size_t KCA_SUM_GROUP = 16;     // signatures per lane and level of the group sums

namespace {
struct KcaCall {
  const uint32_t* com; const uint32_t* pos; const uint8_t* sigs; const uint64_t* sig_off;   // pos / sigs indexed by the offsets as given
  const uint8_t* msgs; const uint64_t* msg_off; const uint64_t* sel_off;
  size_t n_groups;
  const uint8_t* dst; size_t dst_len;
  bool wire;                                                           // sigs holds 32 bytes per entry, the sums leave compressed too
};
}

// One attempt over the groups of A, enqueued: the signature sums' encodings into c->kcagg.out, the rows into c->kcagg.rows (row g
// at sel_off[g] - sel_off[0]), the bits of the groups' equation into c->kcagg.gbits; A.wire: the sums' compressed encodings into
// c->kcagg.wout as well.
static int kca_attempt(blsbn254_ctx* c, const blsbn254_keyset* k, const KcaCall& A, bool fallback) {
  KcaWs& w = c->kcagg;
  const size_t ng = A.n_groups;
  TRY(stage_group_offsets(c, w.goff, A.sig_off, ng));
  const size_t N = w.goff.h[ng], N1 = N ? N : 1, nb = (N + 7) / 8;
  kca_layout(k->cm.tab, A.com, A.sel_off, ng, w.h_wpre, w.h_roff);     // (ctx-owned: the arrays outlive the uploads)
  const size_t n_words = w.h_wpre[ng], row_bytes = w.h_roff[ng];
  TRY(upload(c, w.com, A.com, 4 * ng));
  TRY(upload(c, w.wpre, w.h_wpre.data(), 8 * (ng + 1))); TRY(upload(c, w.roff, w.h_roff.data(), 8 * (ng + 1)));
  const bool scan_wire = A.wire && !fallback;                          // the scan inflates: no 64-byte form of the entries
  HIPCHK(c, w.pos.reserve(4 * N1));
  if (!scan_wire) HIPCHK(c, w.sigs.reserve(64 * N1));
  if (A.wire) HIPCHK(c, w.wire.reserve(32 * N1));
  if (N) {
    TRY(upload(c, w.pos, A.pos + A.sig_off[0], 4 * N));
    if (!A.wire) TRY(upload(c, w.sigs, A.sigs + 64 * A.sig_off[0], 64 * N));
    else {
      TRY(upload(c, w.wire, A.sigs + 32 * A.sig_off[0], 32 * N));
      if (fallback) TRY(g1_inflate_dev(c, (const uint8_t*)w.wire.p, N, (uint8_t*)w.sigs.p));
    }
  }
  const uint32_t* goff = (const uint32_t*)w.goff.d.p;
  const uint4* coms = (const uint4*)k->cm.coms.p;
  const uint32_t* com = (const uint32_t*)w.com.p;
  if (fallback && N) {
    // every entry as the tuple (its key, the group's message, its signature): the registry indices from the member list, the keys
    // by index from the handle, the group's message once per entry (ctx-owned: outlives the upload), the bits into w.vbits
    HIPCHK(c, w.ridx.reserve(4 * N)); HIPCHK(c, w.pks.reserve(128 * N)); HIPCHK(c, w.vbits.reserve(nb + 8));
    TRY(for_chunks(c, N, [&](size_t lo, size_t m) {
      return launch(c, c->stream, "kca_resolve", grid_lanes(m), k_kca_resolve, (const uint32_t*)k->cm.members.p, coms, com, goff, (uint32_t)ng, (const uint32_t*)w.pos.p, m,
                    (uint32_t)lo, (uint32_t*)w.ridx.p);
    }));
    TRY(for_chunks(c, N, [&](size_t lo, size_t m) {
      return launch(c, c->stream, "ka_gather_keys", grid_lanes(8 * m), k_ka_gather_keys, (const uint4*)k->enc.p, (const uint32_t*)w.ridx.p + lo, m, (uint4*)w.pks.p + 8 * lo);
    }));
    w.s_emsgs.clear(); w.s_emoff.assign(1, 0);
    for (size_t g = 0; g < ng; ++g)
      for (uint32_t s = w.goff.h[g]; s < w.goff.h[g + 1]; ++s) {
        if (A.msg_off[g + 1] != A.msg_off[g]) w.s_emsgs.insert(w.s_emsgs.end(), A.msgs + A.msg_off[g], A.msgs + A.msg_off[g + 1]);
        w.s_emoff.push_back(w.s_emsgs.size());
      }
    TRY(stage_msgs(c, w.s_emsgs.data(), w.s_emoff.data(), N));
    TRY(blsbn254_internal_verify_batch_dev_sync(c, (const uint8_t*)w.pks.p, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, (const uint8_t*)w.sigs.p, N, A.dst, A.dst_len,
                                                (uint8_t*)w.vbits.p));
  }
  HIPCHK(c, w.cand.reserve(nb + 8)); HIPCHK(c, w.pts.reserve(27 * N1 * 4)); HIPCHK(c, w.rows.reserve(row_bytes));
  HIPCHK(c, w.gsum.reserve(27 * ng * 4)); HIPCHK(c, w.out.reserve(64 * ng)); HIPCHK(c, w.gbits.reserve((ng + 7) / 8 + 8));
  if (A.wire) HIPCHK(c, w.wout.reserve(32 * ng));
  TRY(for_chunks(c, N, [&](size_t lo, size_t m) {
    if (scan_wire)
      return launch(c, c->stream, "kca_scan_wire", grid_lanes(m), k_kca_scan_wire, (const uint32_t*)k->cm.cvalid.p, coms, com, goff, (uint32_t)ng, (const uint32_t*)w.pos.p,
                    (const uint8_t*)w.wire.p, (const uint8_t*)nullptr, m, (uint32_t)lo, N, (uint8_t*)w.cand.p, (int32_t*)w.pts.p);
    return launch(c, c->stream, "kca_scan", grid_lanes(m), k_kca_scan, (const uint32_t*)k->cm.cvalid.p, coms, com, goff, (uint32_t)ng, (const uint32_t*)w.pos.p,
                  (const uint8_t*)w.sigs.p, fallback ? (const uint8_t*)w.vbits.p : (const uint8_t*)nullptr, m, (uint32_t)lo, N, (uint8_t*)w.cand.p, (int32_t*)w.pts.p);
  }));
  // (the candidate bitmap is complete: every launch of the scan is enqueued before the first row is built)
  TRY(for_chunks(c, n_words, [&](size_t lo, size_t m) {
    return launch(c, c->stream, "kca_rows", grid_lanes(m), k_kca_rows, (const uint32_t*)w.pos.p, (const uint8_t*)w.cand.p, goff, (const uint64_t*)w.wpre.p,
                  (const uint64_t*)w.roff.p, coms, com, (uint32_t)ng, m, (uint64_t)lo, (uint8_t*)w.rows.p);
  }));
  // the signature sums: launches of whole groups, planned up front (a group has at most as many entries as its committee members)
  w.seg.h_start.clear(); w.seg.h_len.clear();
  std::vector<SegLaunch> launches;
  size_t m_max, items_max;
  if (!plan_launches_whole(w.goff.h, ng, c->chunk, KCA_SUM_GROUP, (size_t)-1, launches, w.seg.h_start, w.seg.h_len, &m_max, &items_max)) {
    c->last_error = "internal: group sums do not converge";
    return BLSBN254_E_HIP;
  }
  TRY(seg_stage(c, w.seg, items_max, 27, false));
  for (const SegLaunch& L : launches)
    TRY(seg_run_levels(w.seg, L.levels, {(const int32_t*)w.pts.p + L.lo, N1, nullptr}, {(int32_t*)w.gsum.p + L.ga, ng, nullptr},
                       [&](SegSrc in, const uint32_t* start, const uint32_t* len, size_t runs, SegDst out, bool) {
      return launch(c, c->stream, "g1_seg_sum", grid_lanes(runs), k_g1_seg_sum, in.v, in.stride, (const uint32_t*)nullptr, start, len, runs, out.v, out.stride);
    }));
  if (A.wire) TRY(launch(c, c->stream, "g1p_to_wire", grid_lanes(ng), k_g1p_to_wire, (const int32_t*)w.gsum.p, ng, ng, (uint8_t*)w.out.p, (uint8_t*)w.wout.p));
  else TRY(launch(c, c->stream, "g1p_to_bytes", grid_lanes(ng), k_g1p_to_bytes, (const int32_t*)w.gsum.p, ng, ng, (uint8_t*)w.out.p));
  // the key sums from the rows where they are, by the committee path, then the equation of the committee verify
  TRY(kc_enqueue_call_dev(c, k, A.com, (const uint8_t*)w.rows.p, A.sel_off, ng));
  HIPCHK(c, c->gs_pk.reserve(128 * ng));
  TRY(launch(c, c->stream, "g2p_to_bytes", grid_lanes(ng), k_g2p_to_bytes, (const int32_t*)c->gs_sum.p, ng, (const uint8_t*)c->gs_sum_ok.p, ng, (uint8_t*)c->gs_pk.p, 1));
  uint32_t dl;
  TRY(stage_dst(c, A.dst, A.dst_len, &dl));
  TRY(stage_msgs(c, A.msgs, A.msg_off, ng));               // ONE message per group
  return verify_chunk_dev(c, (const uint8_t*)c->gs_pk.p, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, (const uint8_t*)w.out.p, ng, dl, (uint8_t*)w.gbits.p);
}

// both forms of the entry point; wire: sigs and out_sigs hold 32 bytes per signature
static int kca_checked(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* com, const uint32_t* pos, const uint8_t* sigs, const uint64_t* sig_off,
                       const uint8_t* msgs, const uint64_t* msg_off, const uint64_t* sel_off, size_t n_groups, const uint8_t* dst, size_t dst_len, uint8_t* out_sigs,
                       uint8_t* out_sel, uint8_t* status, bool wire) {
  if (!c || !k || k->ctx != c) return BLSBN254_E_ARG;
  if (n_groups == 0) return 0;
  if (!com || !sig_off || !msg_off || !sel_off || !out_sigs || !out_sel || !status || (dst_len && !dst)) return BLSBN254_E_ARG;
  if (k->cm.tab.com.empty()) { c->last_error = "the key set has no committees (blsbn254_keyset_set_committees)"; return BLSBN254_E_ARG; }
  if (n_groups > c->chunk) { c->last_error = "more groups than one launch chunk"; return BLSBN254_E_ARG; }
  if (check_offsets(sig_off, n_groups)) { c->last_error = "group offsets decrease"; return BLSBN254_E_ARG; }
  if (check_offsets(msg_off, n_groups)) { c->last_error = "message offsets decrease"; return BLSBN254_E_ARG; }
  if (check_offsets(sel_off, n_groups)) { c->last_error = "row offsets decrease"; return BLSBN254_E_ARG; }
  if (!msgs && msg_off[n_groups] != msg_off[0]) return BLSBN254_E_ARG;
  if (sig_off[n_groups] != sig_off[0] && (!pos || !sigs)) return BLSBN254_E_ARG;
  const KcTable& T = k->cm.tab;
  const KcaWalk wk = kca_walk(T, com, pos, sig_off, sel_off, n_groups, MAX_LANES);
  if (wk.code != KCA_OK) {
    const std::string who = "group " + std::to_string(wk.group);
    c->last_error = wk.code == KCA_TOO_MANY ? "more than 2^23 entries in one call"
                  : wk.code == KCA_COM_RANGE ? who + " names committee " + std::to_string(com[wk.group]) + " of " + std::to_string(T.com.size())
                  : wk.code == KCA_ROW_LEN ? who + ": the row must be " + std::to_string(kc_row_bytes(T.com[com[wk.group]].size)) + " bytes"
                  : wk.code == KCA_POS_RANGE ? "entry " + std::to_string(wk.entry - sig_off[0]) + " names no member of its committee"
                  : wk.code == KCA_POS_ORDER ? who + ": positions do not strictly increase"
                  : "group offsets decrease";
    return BLSBN254_E_ARG;
  }
  ENTER(c);
  KcaWs& w = c->kcagg;
  const size_t gb = (n_groups + 7) / 8, total = sel_off[n_groups] - sel_off[0], sb = wire ? 32 : 64;
  const DevBuf& d_out = wire ? w.wout : w.out;                         // the sums as the caller gets them
  const KcaCall A{com, pos, sigs, sig_off, msgs, msg_off, sel_off, n_groups, dst, dst_len, wire};
  TRY(kca_attempt(c, k, A, false));
  w.h_gbits.assign(gb, 0);
  HIPCHK(c, hipMemcpyAsync(out_sigs, d_out.p, sb * n_groups, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(out_sel, w.rows.p, total, hipMemcpyDeviceToHost, c->stream));
  TRY(download(c, w.h_gbits.data(), w.gbits.p, gb));
  // a group whose equation does not hold: the identity and, once the repack has read its candidates off the row, a zero row
  w.fail.clear();
  for (size_t g = 0; g < n_groups; ++g) {
    if ((w.h_gbits[g >> 3] >> (g & 7)) & 1) { status[g] = 0; ++c->stat_kcagg[0]; continue; }
    status[g] = BLSBN254_ST_SHORT;
    g1_identity_out(out_sigs + sb * g, wire);
    const uint8_t *row = out_sel + (sel_off[g] - sel_off[0]), *end = out_sel + (sel_off[g + 1] - sel_off[0]);
    if (std::any_of(row, end, [](uint8_t b) { return b != 0; })) w.fail.push_back(g);
    else ++c->stat_kcagg[3];
  }
  if (w.fail.empty()) return 0;
  // the sub-call over the failing groups' candidates, repacked (ctx-owned: the arrays outlive the asynchronous uploads)
  const size_t nf = w.fail.size();
  kca_repack(w.fail, com, pos, sig_off, sel_off, out_sel, w.sub);
  const size_t Ns = w.sub.pos.size();
  w.s_sigs.resize(sb * Ns);
  for (size_t i = 0; i < Ns; ++i) std::memcpy(w.s_sigs.data() + sb * i, sigs + sb * w.sub.src[i], sb);
  w.s_msgs.clear(); w.s_moff.assign(1, 0);
  for (size_t g : w.fail) {
    std::memset(out_sel + (sel_off[g] - sel_off[0]), 0, sel_off[g + 1] - sel_off[g]);
    if (msg_off[g + 1] != msg_off[g]) w.s_msgs.insert(w.s_msgs.end(), msgs + msg_off[g], msgs + msg_off[g + 1]);
    w.s_moff.push_back(w.s_msgs.size());
  }
  c->stat_kcagg[1] += nf; c->stat_kcagg[2] += Ns;
  const KcaCall B{w.sub.com.data(), w.sub.pos.data(), w.s_sigs.data(), w.sub.off.data(), w.s_msgs.data(), w.s_moff.data(), w.sub.sel_off.data(), nf, dst, dst_len, wire};
  TRY(kca_attempt(c, k, B, true));
  const size_t sub_total = w.sub.sel_off[nf];
  w.s_out.resize(sb * nf); w.s_rows.resize(sub_total); w.h_gbits.assign((nf + 7) / 8, 0);
  HIPCHK(c, hipMemcpyAsync(w.s_out.data(), d_out.p, sb * nf, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(w.s_rows.data(), w.rows.p, sub_total, hipMemcpyDeviceToHost, c->stream));
  TRY(download(c, w.h_gbits.data(), w.gbits.p, (nf + 7) / 8));
  for (size_t j = 0; j < nf; ++j) {
    const size_t g = w.fail[j];
    if (!((w.h_gbits[j >> 3] >> (j & 7)) & 1)) { ++c->stat_kcagg[3]; continue; }
    status[g] = 0;
    std::memcpy(out_sigs + sb * g, w.s_out.data() + sb * j, sb);
    std::memcpy(out_sel + (sel_off[g] - sel_off[0]), w.s_rows.data() + w.sub.sel_off[j], sel_off[g + 1] - sel_off[g]);
  }
  return 0;
}

int blsbn254_keyset_committee_aggregate_checked_batch(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* com, const uint32_t* pos, const uint8_t* sigs,
                                                      const uint64_t* sig_off, const uint8_t* msgs, const uint64_t* msg_off, const uint64_t* sel_off, size_t n_groups,
                                                      const uint8_t* dst, size_t dst_len, uint8_t* out_sigs, uint8_t* out_sel, uint8_t* status) {
  return kca_checked(c, k, com, pos, sigs, sig_off, msgs, msg_off, sel_off, n_groups, dst, dst_len, out_sigs, out_sel, status, false);
}
int blsbn254_keyset_committee_aggregate_checked_batch_compressed(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* com, const uint32_t* pos, const uint8_t* sigs,
                                                                 const uint64_t* sig_off, const uint8_t* msgs, const uint64_t* msg_off, const uint64_t* sel_off,
                                                                 size_t n_groups, const uint8_t* dst, size_t dst_len, uint8_t* out_sigs, uint8_t* out_sel,
                                                                 uint8_t* status) {
  return kca_checked(c, k, com, pos, sigs, sig_off, msgs, msg_off, sel_off, n_groups, dst, dst_len, out_sigs, out_sel, status, true);
}

int blsbn254_keyset_committee_aggregate_stats(blsbn254_ctx* c, uint64_t out[4]) {
  if (!c || !out) return BLSBN254_E_ARG;
  for (int i = 0; i < 4; ++i) out[i] = c->stat_kcagg[i];
  return 0;
}

}  // extern "C"
