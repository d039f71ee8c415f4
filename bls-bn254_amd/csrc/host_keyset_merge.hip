// host_keyset_merge.hip -- checked merge of partial aggregates over a registered key set: from the partial aggregates an
// intermediate node of an aggregation tree receives for one message per group, each an aggregate signature with the bitmap of
// the keys in it, ONE merged (aggregate, bitmap) pair per group, with the bad contributions left out.  Host side of
// include/blsbn254.h; kernels in k_keyset_merge.hip, lane functions in keyset_merge.h, the argument walk and the repack in
// keyset_merge_plan.h; see host_common.h and DESIGN.md 6j.
//
// Two attempts, each ONE pass of enqueued work and one download:
//   optimistic   the signature test of every contribution and its signature as a point (k_km_sig), the greedy selection of
//                disjoint candidates in the order given, a wave per group, which leaves the merged rows (k_km_select), the
//                identity over the points of what was not selected and the used / candidate bitmaps (k_km_points), the
//                signature sums (k_g1_seg_sum by levels, k_g1p_to_bytes), the key sums from the merged rows ON THE DEVICE
//                (ks_enqueue_sums_dev), and ONE verification per group of (key sum, message, signature sum).
//   fallback     only for groups that selected something and failed, EVERY candidate of theirs repacked by the host into a
//                sub-call: each contribution verified on its own, by the key sum of ITS row where the sub-call's rows already
//                are on the device (ks_enqueue_sums_dev over the contribution rows, the group's message once per contribution),
//                then the SAME pass with those bits as the selection's mask -- so the kept contributions are selected and summed
//                again and the one equation decides.  No failing group: nothing is launched.
// c->gs_sum / c->gs_pk serve the per-contribution verification first and the groups' equation after it: stream order keeps the
// two uses apart, and both are reserved for the larger use before the first kernel is enqueued.
// A group's outcome depends on its own inputs only: which attempt served it, where a launch ended and how many groups shared
// the call do not change a byte.
//
// The wire-format form (blsbn254_keyset_merge_checked_batch_compressed) shares this body behind KmCall::wire: the
// contributions' 32-byte signatures are uploaded to w.wire and inflated into w.sigs (k_g1_inflate), where k_km_sig reads them as
// ever -- a contribution that does not inflate is the marker no decoder accepts; the sums leave in both encodings
// (k_g1p_to_wire); the fallback's repack carries 32-byte signatures.
#include "host_common.h"

extern "C" {

static const size_t KM_SUM_GROUP = 16;                      // signatures per lane and level of the group sums
static const uint64_t KM_MAX_ROW_BYTES = (uint64_t)1 << 30; // rows of one call, together

namespace {
struct KmCall {
  const uint8_t* rows; const uint8_t* sigs; const uint64_t* con_off;   // indexed by the offsets as given
  const uint8_t* msgs; const uint64_t* msg_off;
  size_t n_groups;
  const uint8_t* dst; size_t dst_len;
  bool wire;                                                           // sigs holds 32 bytes per contribution, the sums leave compressed too
};
}

// One attempt over the groups of A, enqueued: the signature sums' encodings into c->kmrg.out, the merged rows into c->kmrg.urows,
// the used / candidate bitmaps into c->kmrg.used / cand, the bits of the groups' equation into c->kmrg.gbits; A.wire: the sums'
// compressed encodings into c->kmrg.wout as well.
static int km_attempt(blsbn254_ctx* c, const blsbn254_keyset* k, const KmCall& A, bool fallback) {
  KmWs& w = c->kmrg;
  const size_t ng = A.n_groups, rb = (k->n + 7) / 8;
  TRY(stage_group_offsets(c, w.goff, A.con_off, ng));
  const size_t N = w.goff.h[ng], N1 = N ? N : 1, nb = (N + 7) / 8;
  HIPCHK(c, w.rows.reserve(rb * N1)); HIPCHK(c, w.sigs.reserve(64 * N1));
  if (N) {
    TRY(upload(c, w.rows, A.rows + rb * A.con_off[0], rb * N));
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
  size_t word_launches;
  if (fallback && N) {
    // every contribution as the tuple (the key sum of its row, the group's message, its signature): the group's message once per
    // contribution (ctx-owned: outlives the upload), by launches of at most c->chunk contributions, the bits into w.vbits
    HIPCHK(c, w.vbits.reserve(nb + 8));
    w.s_emsgs.clear(); w.s_emoff.assign(1, 0);
    for (size_t g = 0; g < ng; ++g)
      for (uint32_t s = w.goff.h[g]; s < w.goff.h[g + 1]; ++s) {
        if (A.msg_off[g + 1] != A.msg_off[g]) w.s_emsgs.insert(w.s_emsgs.end(), A.msgs + A.msg_off[g], A.msgs + A.msg_off[g + 1]);
        w.s_emoff.push_back(w.s_emsgs.size());
      }
    TRY(for_chunks(c, N, [&](size_t lo, size_t m) {
      TRY(ks_enqueue_sums_dev(c, k, (const uint8_t*)w.rows.p + lo * rb, m, &word_launches));
      TRY(launch(c, c->stream, "g2p_to_bytes", grid_lanes(m), k_g2p_to_bytes, (const int32_t*)c->gs_sum.p, m, (const uint8_t*)c->gs_sum_ok.p, m, (uint8_t*)c->gs_pk.p, 1));
      TRY(stage_msgs(c, w.s_emsgs.data(), w.s_emoff.data() + lo, m));
      return verify_chunk_dev(c, (const uint8_t*)c->gs_pk.p, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, (const uint8_t*)w.sigs.p + 64 * lo, m, dl,
                              (uint8_t*)w.vbits.p + (lo >> 3));
    }));
  }
  HIPCHK(c, w.sig_ok.reserve(N1)); HIPCHK(c, w.flags.reserve(N1)); HIPCHK(c, w.used.reserve(nb + 8)); HIPCHK(c, w.cand.reserve(nb + 8));
  HIPCHK(c, w.pts.reserve(27 * N1 * 4)); HIPCHK(c, w.urows.reserve(rb * ng));
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
    TRY(launch(c, c->stream, "km_select", grid_lanes(64 * m), k_km_select, (const uint8_t*)w.rows.p, (const uint8_t*)w.sig_ok.p,
               fallback ? (const uint8_t*)w.vbits.p : (const uint8_t*)nullptr, goff, (const uint32_t*)k->vwords.p, (uint32_t)k->n, lo, m, (uint8_t*)w.flags.p,
               (uint8_t*)w.urows.p));
  }
  TRY(for_chunks(c, N, [&](size_t lo, size_t m) {
    return launch(c, c->stream, "km_points", grid_lanes(m), k_km_points, (const uint8_t*)w.flags.p, m, (uint32_t)lo, N, (int32_t*)w.pts.p, (uint8_t*)w.used.p,
                  (uint8_t*)w.cand.p);
  }));
  // the signature sums: launches of whole groups, planned up front
  w.seg.h_start.clear(); w.seg.h_len.clear();
  std::vector<SegLaunch> launches;
  size_t m_max, items_max;
  if (!plan_launches_whole(w.goff.h, ng, c->chunk, KM_SUM_GROUP, (size_t)-1, launches, w.seg.h_start, w.seg.h_len, &m_max, &items_max)) {
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
  // the key sums from the merged rows where they are, then the equation of blsbn254_keyset_fast_aggregate_verify_batch
  TRY(ks_enqueue_sums_dev(c, k, (const uint8_t*)w.urows.p, ng, &word_launches));
  TRY(launch(c, c->stream, "g2p_to_bytes", grid_lanes(ng), k_g2p_to_bytes, (const int32_t*)c->gs_sum.p, ng, (const uint8_t*)c->gs_sum_ok.p, ng, (uint8_t*)c->gs_pk.p, 1));
  TRY(stage_msgs(c, A.msgs, A.msg_off, ng));               // ONE message per group
  return verify_chunk_dev(c, (const uint8_t*)c->gs_pk.p, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, (const uint8_t*)w.out.p, ng, dl, (uint8_t*)w.gbits.p);
}

static inline bool km_bit(const std::vector<uint8_t>& bm, size_t i) { return (bm[i >> 3] >> (i & 7)) & 1; }

// both forms of the entry point; wire: sigs and out_sigs hold 32 bytes per signature
static int km_checked(blsbn254_ctx* c, const blsbn254_keyset* k, const uint8_t* rows, const uint8_t* sigs, const uint64_t* con_off, const uint8_t* msgs,
                      const uint64_t* msg_off, size_t n_groups, const uint8_t* dst, size_t dst_len, uint8_t* out_sigs, uint8_t* out_sel, uint8_t* used,
                      uint8_t* status, bool wire) {
  if (!c) return BLSBN254_E_ARG;
  if (!k) { c->last_error = "a NULL argument"; return BLSBN254_E_ARG; }
  if (k->ctx != c) { c->last_error = "the key set belongs to another context"; return BLSBN254_E_ARG; }
  if (n_groups == 0) return 0;
  if (!con_off || !msg_off || !out_sigs || !out_sel || !used || !status || (dst_len && !dst)) { c->last_error = "a NULL argument"; return BLSBN254_E_ARG; }
  if (n_groups > c->chunk) { c->last_error = "more groups than one launch chunk"; return BLSBN254_E_ARG; }
  if (check_offsets(con_off, n_groups)) { c->last_error = "contribution offsets decrease"; return BLSBN254_E_ARG; }
  if (check_offsets(msg_off, n_groups)) { c->last_error = "message offsets decrease"; return BLSBN254_E_ARG; }
  if (!msgs && msg_off[n_groups] != msg_off[0]) { c->last_error = "a NULL argument"; return BLSBN254_E_ARG; }
  if (con_off[n_groups] != con_off[0] && (!rows || !sigs)) { c->last_error = "a NULL argument"; return BLSBN254_E_ARG; }
  const KmWalk wk = km_walk(rows, con_off, n_groups, k->n, MAX_LANES, KM_MAX_ROW_BYTES);
  if (wk.code != KM_OK) {
    c->last_error = wk.code == KM_TOO_MANY ? "more than 2^23 contributions in one call"
                  : wk.code == KM_ROWS_TOO_LARGE ? "more than 2^30 bytes of rows in one call"
                  : wk.code == KM_ROW_PAD ? "contribution " + std::to_string(wk.con - con_off[0]) + " sets a bit past the last key"
                  : "contribution offsets decrease";
    return BLSBN254_E_ARG;
  }
  ENTER(c);
  KmWs& w = c->kmrg;
  const size_t rb = (k->n + 7) / 8, gb = (n_groups + 7) / 8, sb = wire ? 32 : 64;
  const size_t N = (size_t)(con_off[n_groups] - con_off[0]), nb = (N + 7) / 8;
  const DevBuf& d_out = wire ? w.wout : w.out;                         // the sums as the caller gets them
  const KmCall A{rows, sigs, con_off, msgs, msg_off, n_groups, dst, dst_len, wire};
  TRY(km_attempt(c, k, A, false));
  w.h_gbits.assign(gb, 0); w.h_used.assign(nb + 1, 0); w.h_cand.assign(nb + 1, 0);
  HIPCHK(c, hipMemcpyAsync(out_sigs, d_out.p, sb * n_groups, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(out_sel, w.urows.p, rb * n_groups, hipMemcpyDeviceToHost, c->stream));
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
    if (km_bit(w.h_gbits, g)) {
      status[g] = 0; ++c->stat_kmrg[0];
      for (uint64_t s = con_off[g] - con_off[0]; s < con_off[g + 1] - con_off[0]; ++s)
        if (km_bit(w.h_used, s)) used[s >> 3] |= (uint8_t)(1u << (s & 7));
      continue;
    }
    status[g] = BLSBN254_ST_SHORT;
    g1_identity_out(out_sigs + sb * g, wire);
    uint8_t* row = out_sel + g * rb;
    if (std::any_of(row, row + rb, [](uint8_t b) { return b != 0; })) w.fail.push_back(g);
    else ++c->stat_kmrg[3];
    std::memset(row, 0, rb);
  }
  if (w.fail.empty()) return 0;
  // the sub-call over the failing groups' candidates, repacked (ctx-owned: the arrays outlive the asynchronous uploads)
  const size_t nf = w.fail.size();
  km_repack(w.fail, rows, sigs, con_off, w.h_cand.data(), rb, w.sub, sb);
  const size_t Ns = w.sub.pos.size();
  w.s_msgs.clear(); w.s_moff.assign(1, 0);
  for (size_t g : w.fail) {
    if (msg_off[g + 1] != msg_off[g]) w.s_msgs.insert(w.s_msgs.end(), msgs + msg_off[g], msgs + msg_off[g + 1]);
    w.s_moff.push_back(w.s_msgs.size());
  }
  c->stat_kmrg[1] += nf; c->stat_kmrg[2] += Ns;
  const KmCall B{w.sub.rows.data(), w.sub.sigs.data(), w.sub.off.data(), w.s_msgs.data(), w.s_moff.data(), nf, dst, dst_len, wire};
  TRY(km_attempt(c, k, B, true));
  const size_t nbs = (Ns + 7) / 8;
  w.s_out.resize(sb * nf); w.s_rows.resize(rb * nf); w.h_gbits.assign((nf + 7) / 8, 0); w.h_used.assign(nbs + 1, 0);
  HIPCHK(c, hipMemcpyAsync(w.s_out.data(), d_out.p, sb * nf, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(w.s_rows.data(), w.urows.p, rb * nf, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(w.h_used.data(), w.used.p, nbs, hipMemcpyDeviceToHost, c->stream));
  TRY(download(c, w.h_gbits.data(), w.gbits.p, (nf + 7) / 8));
  for (size_t j = 0; j < nf; ++j) {
    const size_t g = w.fail[j];
    if (!km_bit(w.h_gbits, j)) { ++c->stat_kmrg[3]; continue; }
    status[g] = 0;
    std::memcpy(out_sigs + sb * g, w.s_out.data() + sb * j, sb);
    std::memcpy(out_sel + g * rb, w.s_rows.data() + rb * j, rb);
    for (uint64_t i = w.sub.off[j]; i < w.sub.off[j + 1]; ++i)
      if (km_bit(w.h_used, i)) { const uint64_t s = w.sub.pos[i] - con_off[0]; used[s >> 3] |= (uint8_t)(1u << (s & 7)); }
  }
  return 0;
}

int blsbn254_keyset_merge_checked_batch(blsbn254_ctx* c, const blsbn254_keyset* k, const uint8_t* rows, const uint8_t* sigs, const uint64_t* con_off,
                                        const uint8_t* msgs, const uint64_t* msg_off, size_t n_groups, const uint8_t* dst, size_t dst_len,
                                        uint8_t* out_sigs, uint8_t* out_sel, uint8_t* used, uint8_t* status) {
  return km_checked(c, k, rows, sigs, con_off, msgs, msg_off, n_groups, dst, dst_len, out_sigs, out_sel, used, status, false);
}
int blsbn254_keyset_merge_checked_batch_compressed(blsbn254_ctx* c, const blsbn254_keyset* k, const uint8_t* rows, const uint8_t* sigs, const uint64_t* con_off,
                                                   const uint8_t* msgs, const uint64_t* msg_off, size_t n_groups, const uint8_t* dst, size_t dst_len,
                                                   uint8_t* out_sigs, uint8_t* out_sel, uint8_t* used, uint8_t* status) {
  return km_checked(c, k, rows, sigs, con_off, msgs, msg_off, n_groups, dst, dst_len, out_sigs, out_sel, used, status, true);
}

int blsbn254_keyset_merge_stats(blsbn254_ctx* c, uint64_t out[4]) {
  if (!c || !out) return BLSBN254_E_ARG;
  for (int i = 0; i < 4; ++i) out[i] = c->stat_kmrg[i];
  return 0;
}

}  // extern "C"
