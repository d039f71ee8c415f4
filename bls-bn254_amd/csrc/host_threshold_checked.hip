// host_threshold_checked.hip -- the checked threshold combine over ragged groups: from a group's Feldman commitments, its
// message and the n_g >= t_g partial signatures received, the group signature, with the bad partials left out.  Host side of
// include/blsbn254.h; kernels in k_threshold_checked.hip; see host_common.h and DESIGN.md 6g.
//
// Two attempts, each ONE pass of enqueued work, one download and one synchronisation:
//   optimistic   commitments and ids tested once, the candidate bit of every partial signature (k_tc_scan), the first t_g
//                candidates of every group compacted on the device (k_tc_select), the combine of host_threshold_batch.hip on
//                the compacted arrays (th_enqueue_dev), and ONE verification per group of the result under C_0
//                (k_tc_gather_c0, the verify pipeline with one message per group).
//   fallback     only for groups whose result did not verify, repacked by the host (it holds their arrays) into a sub-call:
//                every share verified against its key share (td_verify_shares_enqueue), the first t_g candidates that verify
//                compacted by the same kernel, the same combine.  Partial signatures that verify individually interpolate to
//                [f(0)] H(m): that result is not verified again.  No failing group: nothing is launched.
// A group's outcome depends on its own inputs only: which attempt served it, where a launch ended and how many groups shared
// the call do not change a byte.
#include "host_common.h"

extern "C" {

static const uint32_t TC_MARK_SCALAR = 1u, TC_MARK_POINT = 2u, TC_MARK_SHORT = 4u;   // threshold_deal.h / threshold_checked.h: the bits of a group's mark word

namespace {
struct TcCall {
  const uint8_t *commitments, *ids, *sigs, *msgs;
  const uint64_t *coef_off, *id_off, *msg_off;
  size_t n_groups;
  const uint8_t* dst; size_t dst_len;
};
}
static inline uint8_t tc_code(uint32_t marks) {
  return (marks & TC_MARK_SCALAR) ? BLSBN254_ERR_SCALAR : (marks & TC_MARK_POINT) ? BLSBN254_ERR_G2 : (marks & TC_MARK_SHORT) ? BLSBN254_ST_SHORT : 0;
}

// One attempt over the groups of A, enqueued: the combined signatures into c->thb.out, the used bits into c->tc.used, the marks
// into c->tc.gstat; the optimistic one also the bits of the groups' verification into c->tc.gbits.
static int tc_attempt(blsbn254_ctx* c, const TcCall& A, bool fallback) {
  TcWs& w = c->tc;
  const size_t ng = A.n_groups;
  TRY(stage_group_offsets(c, w.goff, A.id_off, ng)); TRY(stage_group_offsets(c, w.coff, A.coef_off, ng));
  const size_t N = w.goff.h[ng], T = w.coff.h[ng], T1 = T ? T : 1, nb = (N + 7) / 8;
  // the fallback's per-share verification first: it stages the sub-call's commitments, messages and partial signatures in the
  // buffers of its own pipelines and leaves the shares' bits in c->bitmap
  if (fallback) TRY(td_verify_shares_enqueue(c, A.commitments, A.coef_off, A.ids, A.sigs, A.id_off, A.msgs, A.msg_off, ng, A.dst, A.dst_len));
  HIPCHK(c, w.gstat.reserve(4 * ng)); HIPCHK(c, w.st.reserve(ng));
  HIPCHK(c, w.cand.reserve(nb + 8)); HIPCHK(c, w.used.reserve(nb + 8)); HIPCHK(c, w.c_ids.reserve(32 * T1)); HIPCHK(c, w.c_sigs.reserve(64 * T1));
  HIPCHK(c, hipMemsetAsync(w.gstat.p, 0, 4 * ng, c->stream));
  HIPCHK(c, hipMemsetAsync(w.c_ids.p, 0, 32 * T1, c->stream)); HIPCHK(c, hipMemsetAsync(w.c_sigs.p, 0, 64 * T1, c->stream));
  const uint32_t* goff = (const uint32_t*)w.goff.d.p; const uint32_t* coff = (const uint32_t*)w.coff.d.p;
  uint32_t* gstat = (uint32_t*)w.gstat.p;
  TdlWs& d = c->tdl;                                     // the commitments: staged and tested where the dealing side does it
  if (!fallback) TRY(td_stage_commitments(c, A.commitments, A.coef_off, ng));
  if (N) {
    const size_t m1 = std::min(N, c->chunk);
    HIPCHK(c, c->th.x.reserve(9 * m1 * 4)); HIPCHK(c, c->status.reserve(m1));
    TRY(upload(c, w.ids, A.ids + 32 * A.id_off[0], 32 * N));
    TRY(upload(c, w.sigs, A.sigs + 64 * A.id_off[0], 64 * N));
    TRY(for_chunks(c, N, [&](size_t lo, size_t m) {
      TRY(launch(c, c->stream, "fr_decode", grid_lanes(m), k_fr_decode, (const uint8_t*)w.ids.p + 32 * lo, m, (int32_t*)c->th.x.p, (uint8_t*)c->status.p));
      return launch(c, c->stream, "tc_scan", grid_lanes(m), k_tc_scan, (const uint8_t*)w.ids.p, (const uint8_t*)w.sigs.p, (const uint8_t*)c->status.p, m, (uint32_t)lo, goff,
                    (uint32_t)ng, gstat, (uint8_t*)w.cand.p);
    }));
  }
  // (the fallback's groups passed both tests in the optimistic attempt)
  if (!fallback) TRY(launch(c, c->stream, "td_finish", grid_lanes(ng), k_td_finish, gstat, ng, coff, (const uint8_t*)d.c_ok.p, (const uint8_t*)d.c_sub.p, TC_MARK_POINT,
                            (uint8_t*)w.st.p));
  TRY(for_chunks(c, N, [&](size_t lo, size_t m) {
    return launch(c, c->stream, "tc_select", grid_lanes(m), k_tc_select, (const uint8_t*)w.cand.p, fallback ? (const uint8_t*)c->bitmap.p : (const uint8_t*)nullptr, m, (uint32_t)lo,
                  goff, coff, (uint32_t)ng, gstat, (const uint32_t*)w.ids.p, (const uint32_t*)w.sigs.p, (uint32_t*)w.c_ids.p, (uint32_t*)w.c_sigs.p, (uint8_t*)w.used.p);
  }));
  // the compacted layout has exactly t_g slots per group: its group offsets ARE the coefficient offsets
  TRY(th_enqueue_dev(c, (const uint8_t*)w.c_ids.p, (const uint8_t*)w.c_sigs.p, A.coef_off, ng));
  if (fallback) return 0;
  HIPCHK(c, w.keys.reserve(128 * ng)); HIPCHK(c, w.gbits.reserve((ng + 7) / 8 + 8));
  TRY(launch(c, c->stream, "tc_gather_c0", grid_lanes(ng), k_tc_gather_c0, (const uint32_t*)d.coef.p, coff, goff, ng, gstat, (uint32_t*)w.keys.p));
  TRY(stage_msgs(c, A.msgs, A.msg_off, ng));             // ONE message per group
  return blsbn254_internal_verify_batch_dev_sync(c, (const uint8_t*)w.keys.p, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, (const uint8_t*)c->thb.out.p, ng, A.dst,
                                                 A.dst_len, (uint8_t*)w.gbits.p);
}

int blsbn254_threshold_combine_checked_batch(blsbn254_ctx* c, const uint8_t* commitments, const uint64_t* coef_off, const uint8_t* ids, const uint8_t* partial_sigs,
                                             const uint64_t* id_off, const uint8_t* msgs, const uint64_t* msg_off, size_t n_groups, const uint8_t* dst, size_t dst_len,
                                             uint8_t* out_sigs, uint8_t* used_bitmap, uint8_t* status) {
  if (!c) return BLSBN254_E_ARG;
  if (n_groups == 0) return 0;
  int rc = td_args(c, commitments, coef_off, ids, id_off, n_groups, used_bitmap, status);
  if (rc) return rc;
  if (!out_sigs) return BLSBN254_E_ARG;
  TRY(td_msg_args(c, partial_sigs, id_off, msgs, msg_off, n_groups, dst, dst_len));
  const size_t N = (size_t)(id_off[n_groups] - id_off[0]), nb = (N + 7) / 8;
  for (size_t g = 0; g < n_groups; ++g)
    if (id_off[g + 1] - id_off[g] > th_batch_tbig()) { c->last_error = "a group of more shares than the lane-per-share combine serves"; return BLSBN254_E_ARG; }
  ENTER(c);
  TcWs& w = c->tc;
  const TcCall A{commitments, ids, partial_sigs, msgs, coef_off, id_off, msg_off, n_groups, dst, dst_len};
  TRY(tc_attempt(c, A, false));
  w.h_gstat.resize(n_groups); w.h_gbits.assign((n_groups + 7) / 8, 0);
  HIPCHK(c, hipMemcpyAsync(out_sigs, c->thb.out.p, 64 * n_groups, hipMemcpyDeviceToHost, c->stream));
  if (N) HIPCHK(c, hipMemcpyAsync(used_bitmap, w.used.p, nb, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(w.h_gbits.data(), w.gbits.p, (n_groups + 7) / 8, hipMemcpyDeviceToHost, c->stream));
  TRY(download(c, w.h_gstat.data(), w.gstat.p, 4 * n_groups));
  // a group that carries a mark, or whose signature did not verify: the identity and no used bit (the fallback sets its own)
  w.fail.clear();
  for (size_t g = 0; g < n_groups; ++g) {
    const uint8_t code = tc_code(w.h_gstat[g]);
    const bool good = (w.h_gbits[g >> 3] >> (g & 7)) & 1;
    status[g] = code;
    if (!code && good) { ++c->tc.stat[0]; continue; }
    if (code == BLSBN254_ST_SHORT) ++c->tc.stat[3];
    if (!code) w.fail.push_back(g);
    g1_identity_bytes(out_sigs + 64 * g);
    for (uint64_t s = id_off[g] - id_off[0]; s < id_off[g + 1] - id_off[0]; ++s) used_bitmap[s >> 3] &= (uint8_t)~(1u << (s & 7));
  }
  if (w.fail.empty()) return 0;
  // the sub-call over the failing groups, repacked (ctx-owned: the arrays outlive the asynchronous uploads)
  const size_t k = w.fail.size();
  w.s_commit.clear(); w.s_ids.clear(); w.s_sigs.clear(); w.s_msgs.clear();
  w.s_coff.assign(1, 0); w.s_goff.assign(1, 0); w.s_moff.assign(1, 0);
  for (size_t g : w.fail) {
    w.s_commit.insert(w.s_commit.end(), commitments + 128 * coef_off[g], commitments + 128 * coef_off[g + 1]);
    w.s_ids.insert(w.s_ids.end(), ids + 32 * id_off[g], ids + 32 * id_off[g + 1]);
    w.s_sigs.insert(w.s_sigs.end(), partial_sigs + 64 * id_off[g], partial_sigs + 64 * id_off[g + 1]);
    if (msg_off[g + 1] != msg_off[g]) w.s_msgs.insert(w.s_msgs.end(), msgs + msg_off[g], msgs + msg_off[g + 1]);
    w.s_coff.push_back(w.s_commit.size() / 128); w.s_goff.push_back(w.s_ids.size() / 32); w.s_moff.push_back(w.s_msgs.size());
  }
  const size_t Ns = (size_t)w.s_goff[k];
  c->tc.stat[1] += k; c->tc.stat[2] += Ns;
  const TcCall B{w.s_commit.data(), w.s_ids.data(), w.s_sigs.data(), w.s_msgs.data(), w.s_coff.data(), w.s_goff.data(), w.s_moff.data(), k, dst, dst_len};
  TRY(tc_attempt(c, B, true));
  w.s_out.resize(64 * k); w.s_used.resize((Ns + 7) / 8); w.h_gstat.resize(k);
  HIPCHK(c, hipMemcpyAsync(w.s_out.data(), c->thb.out.p, 64 * k, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(w.s_used.data(), w.used.p, (Ns + 7) / 8, hipMemcpyDeviceToHost, c->stream));
  TRY(download(c, w.h_gstat.data(), w.gstat.p, 4 * k));
  for (size_t j = 0; j < k; ++j) {
    const size_t g = w.fail[j];
    const uint8_t code = tc_code(w.h_gstat[j]);
    status[g] = code;
    if (code) { ++c->tc.stat[3]; continue; }
    std::memcpy(out_sigs + 64 * g, w.s_out.data() + 64 * j, 64);
    const uint64_t base = id_off[g] - id_off[0];
    for (uint64_t i = 0; i < id_off[g + 1] - id_off[g]; ++i) {
      const uint64_t s = w.s_goff[j] + i;
      if ((w.s_used[s >> 3] >> (s & 7)) & 1) used_bitmap[(base + i) >> 3] |= (uint8_t)(1u << ((base + i) & 7));
    }
  }
  return 0;
}

int blsbn254_threshold_checked_stats(blsbn254_ctx* c, uint64_t out[4]) { return COPY_STATS(c, tc.stat, 4, out); }

}  // extern "C"
