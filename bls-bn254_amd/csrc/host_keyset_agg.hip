// host_keyset_agg.hip -- checked signature aggregation over a registered key set: from the individual signatures of committee
// members on one message per group, the aggregate signature and the participation row that
// blsbn254_keyset_fast_aggregate_verify_batch consumes, with the bad signatures left out.  Host side of include/blsbn254.h;
// kernels in k_keyset_agg.hip, lane functions in keyset_agg.h, the argument walk and the repack in keyset_agg_plan.h; see
// host_common.h and DESIGN.md 6i.
//
// Two attempts, each ONE pass of enqueued work and one download:
//   optimistic   the candidate bit of every entry and its signature as a point (k_ka_scan), the groups' rows from those bits
//                (k_ka_rows), the signature sums (k_g1_seg_sum by levels, k_g1p_to_bytes), the key sums from the rows ON THE
//                DEVICE (ks_enqueue_sums_dev), and ONE verification per group of (key sum, message, signature sum).
//   fallback     only for groups that had a candidate and failed, their candidates repacked by the host into a sub-call: every
//                entry's key gathered from the handle's encodings (k_ka_gather_keys), every signature verified on its own
//                (the verify_batch pipeline, the group's message once per entry), then the SAME pass with those bits as the
//                scan's mask -- so the kept entries are summed again and the one equation decides.  No failing group: nothing
//                is launched.
// A group's outcome depends on its own inputs only: which attempt served it, where a launch ended and how many groups shared
// the call do not change a byte.
//
// The wire-format form (blsbn254_keyset_aggregate_checked_batch_compressed) shares this body behind KaCall::wire:
// 32-byte signatures in, 32-byte sums out.  Its optimistic attempt uploads the 32 N bytes to w.wire and scans them where they
// are (k_ka_scan_wire inflates its own entry; no 64 N buffer exists); its sums leave in both encodings (k_g1p_to_wire: 64 bytes
// for the equation, 32 for the caller).  Its fallback repacks 32-byte entries, inflates them into w.sigs (k_g1_inflate) and goes
// on as above: the per-signature verification reads the 64-byte form.
#include "host_common.h"

extern "C" {

static const size_t KA_SUM_GROUP = 16;      // signatures per lane and level of the group sums

namespace {
struct KaCall {
  const uint32_t* idx; const uint8_t* sigs; const uint64_t* sig_off;   // indexed by the offsets as given
  const uint8_t* msgs; const uint64_t* msg_off;
  size_t n_groups;
  const uint8_t* dst; size_t dst_len;
  bool wire;                                                           // sigs holds 32 bytes per entry, the sums leave compressed too
};
}

// One attempt over the groups of A, enqueued: the signature sums' encodings into c->kagg.out, the rows into c->kagg.rows, the
// bits of the groups' equation into c->kagg.gbits; A.wire: the sums' compressed encodings into c->kagg.wout as well.
static int ka_attempt(blsbn254_ctx* c, const blsbn254_keyset* k, const KaCall& A, bool fallback) {
  KaggWs& w = c->kagg;
  const size_t ng = A.n_groups, rb = (k->n + 7) / 8, W = (k->n + 31) / 32;
  TRY(stage_group_offsets(c, w.goff, A.sig_off, ng));
  const size_t N = w.goff.h[ng], N1 = N ? N : 1, nb = (N + 7) / 8;
  const bool scan_wire = A.wire && !fallback;                          // the scan inflates: no 64-byte form of the entries
  HIPCHK(c, w.idx.reserve(4 * N1));
  if (!scan_wire) HIPCHK(c, w.sigs.reserve(64 * N1));
  if (A.wire) HIPCHK(c, w.wire.reserve(32 * N1));
  if (N) {
    TRY(upload(c, w.idx, A.idx + A.sig_off[0], 4 * N));
    if (!A.wire) TRY(upload(c, w.sigs, A.sigs + 64 * A.sig_off[0], 64 * N));
    else {
      TRY(upload(c, w.wire, A.sigs + 32 * A.sig_off[0], 32 * N));
      if (fallback) TRY(g1_inflate_dev(c, (const uint8_t*)w.wire.p, N, (uint8_t*)w.sigs.p));
    }
  }
  if (fallback && N) {
    // every entry as the tuple (its key, the group's message, its signature): the keys by index from the handle, the group's
    // message once per entry (ctx-owned: outlives the upload), the bits into w.vbits
    HIPCHK(c, w.pks.reserve(128 * N)); HIPCHK(c, w.vbits.reserve(nb + 8));
    TRY(for_chunks(c, N, [&](size_t lo, size_t m) {
      return launch(c, c->stream, "ka_gather_keys", grid_lanes(8 * m), k_ka_gather_keys, (const uint4*)k->enc.p, (const uint32_t*)w.idx.p + lo, m, (uint4*)w.pks.p + 8 * lo);
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
  HIPCHK(c, w.cand.reserve(nb + 8)); HIPCHK(c, w.pts.reserve(27 * N1 * 4)); HIPCHK(c, w.rows.reserve(rb * ng));
  HIPCHK(c, w.gsum.reserve(27 * ng * 4)); HIPCHK(c, w.out.reserve(64 * ng)); HIPCHK(c, w.gbits.reserve((ng + 7) / 8 + 8));
  const uint32_t* goff = (const uint32_t*)w.goff.d.p;
  if (A.wire) HIPCHK(c, w.wout.reserve(32 * ng));
  TRY(for_chunks(c, N, [&](size_t lo, size_t m) {
    if (scan_wire)
      return launch(c, c->stream, "ka_scan_wire", grid_lanes(m), k_ka_scan_wire, (const uint8_t*)k->valid.p, (const uint32_t*)w.idx.p, (const uint8_t*)w.wire.p,
                    (const uint8_t*)nullptr, m, (uint32_t)lo, N, (uint8_t*)w.cand.p, (int32_t*)w.pts.p);
    return launch(c, c->stream, "ka_scan", grid_lanes(m), k_ka_scan, (const uint8_t*)k->valid.p, (const uint32_t*)w.idx.p, (const uint8_t*)w.sigs.p,
                  fallback ? (const uint8_t*)w.vbits.p : (const uint8_t*)nullptr, m, (uint32_t)lo, N, (uint8_t*)w.cand.p, (int32_t*)w.pts.p);
  }));
  // (the candidate bitmap is complete: every launch of the scan is enqueued before the first row is built)
  TRY(for_chunks(c, ng * W, [&](size_t lo, size_t m) {
    return launch(c, c->stream, "ka_rows", grid_lanes(m), k_ka_rows, (const uint32_t*)w.idx.p, (const uint8_t*)w.cand.p, goff, m, lo, (uint32_t)k->n, (uint8_t*)w.rows.p);
  }));
  // the signature sums: launches of whole groups, planned up front (a group has at most n_keys <= 65536 entries)
  w.seg.h_start.clear(); w.seg.h_len.clear();
  std::vector<SegLaunch> launches;
  size_t m_max, items_max;
  if (!plan_launches_whole(w.goff.h, ng, c->chunk, KA_SUM_GROUP, (size_t)-1, launches, w.seg.h_start, w.seg.h_len, &m_max, &items_max)) {
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
  // the key sums from the rows where they are, then the equation of blsbn254_keyset_fast_aggregate_verify_batch
  size_t word_launches;
  TRY(ks_enqueue_sums_dev(c, k, (const uint8_t*)w.rows.p, ng, &word_launches));
  HIPCHK(c, c->gs_pk.reserve(128 * ng));
  TRY(launch(c, c->stream, "g2p_to_bytes", grid_lanes(ng), k_g2p_to_bytes, (const int32_t*)c->gs_sum.p, ng, (const uint8_t*)c->gs_sum_ok.p, ng, (uint8_t*)c->gs_pk.p, 1));
  uint32_t dl;
  TRY(stage_dst(c, A.dst, A.dst_len, &dl));
  TRY(stage_msgs(c, A.msgs, A.msg_off, ng));               // ONE message per group
  return verify_chunk_dev(c, (const uint8_t*)c->gs_pk.p, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, (const uint8_t*)w.out.p, ng, dl, (uint8_t*)w.gbits.p);
}

// both forms of the entry point; wire: sigs and out_sigs hold 32 bytes per signature
static int ka_checked(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* idx, const uint8_t* sigs, const uint64_t* sig_off, const uint8_t* msgs,
                      const uint64_t* msg_off, size_t n_groups, const uint8_t* dst, size_t dst_len, uint8_t* out_sigs, uint8_t* out_sel, uint8_t* status, bool wire) {
  if (!c || !k || k->ctx != c) return BLSBN254_E_ARG;
  if (n_groups == 0) return 0;
  if (!sig_off || !msg_off || !out_sigs || !out_sel || !status || (dst_len && !dst)) return BLSBN254_E_ARG;
  if (n_groups > c->chunk) { c->last_error = "more groups than one launch chunk"; return BLSBN254_E_ARG; }
  if (check_offsets(sig_off, n_groups)) { c->last_error = "group offsets decrease"; return BLSBN254_E_ARG; }
  if (check_offsets(msg_off, n_groups)) { c->last_error = "message offsets decrease"; return BLSBN254_E_ARG; }
  if (!msgs && msg_off[n_groups] != msg_off[0]) return BLSBN254_E_ARG;
  if (sig_off[n_groups] != sig_off[0] && (!idx || !sigs)) return BLSBN254_E_ARG;
  const KaWalk wk = ka_walk(idx, sig_off, n_groups, k->n, MAX_LANES);
  if (wk.code != KA_OK) {
    c->last_error = wk.code == KA_TOO_MANY ? "more than 2^23 entries in one call"
                  : wk.code == KA_IDX_RANGE ? "entry " + std::to_string(wk.entry - sig_off[0]) + " names no key of the set"
                  : wk.code == KA_IDX_ORDER ? "group " + std::to_string(wk.group) + ": key indices do not strictly increase"
                  : "group offsets decrease";
    return BLSBN254_E_ARG;
  }
  ENTER(c);
  KaggWs& w = c->kagg;
  const size_t rb = (k->n + 7) / 8, gb = (n_groups + 7) / 8, sb = wire ? 32 : 64;
  const DevBuf& d_out = wire ? w.wout : w.out;                         // the sums as the caller gets them
  const KaCall A{idx, sigs, sig_off, msgs, msg_off, n_groups, dst, dst_len, wire};
  TRY(ka_attempt(c, k, A, false));
  w.h_gbits.assign(gb, 0);
  HIPCHK(c, hipMemcpyAsync(out_sigs, d_out.p, sb * n_groups, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(out_sel, w.rows.p, rb * n_groups, hipMemcpyDeviceToHost, c->stream));
  TRY(download(c, w.h_gbits.data(), w.gbits.p, gb));
  // a group whose equation does not hold: the identity and, once the repack has read its candidates off the row, a zero row
  w.fail.clear();
  for (size_t g = 0; g < n_groups; ++g) {
    if ((w.h_gbits[g >> 3] >> (g & 7)) & 1) { status[g] = 0; ++c->stat_kagg[0]; continue; }
    status[g] = BLSBN254_ST_SHORT;
    g1_identity_out(out_sigs + sb * g, wire);
    const uint8_t* row = out_sel + g * rb;
    if (std::any_of(row, row + rb, [](uint8_t b) { return b != 0; })) w.fail.push_back(g);
    else ++c->stat_kagg[3];
  }
  if (w.fail.empty()) return 0;
  // the sub-call over the failing groups' candidates, repacked (ctx-owned: the arrays outlive the asynchronous uploads)
  const size_t nf = w.fail.size();
  ka_repack(w.fail, idx, sig_off, out_sel, rb, w.sub);
  const size_t Ns = w.sub.idx.size();
  w.s_sigs.resize(sb * Ns);
  for (size_t i = 0; i < Ns; ++i) std::memcpy(w.s_sigs.data() + sb * i, sigs + sb * w.sub.pos[i], sb);
  w.s_msgs.clear(); w.s_moff.assign(1, 0);
  for (size_t g : w.fail) {
    std::memset(out_sel + g * rb, 0, rb);
    if (msg_off[g + 1] != msg_off[g]) w.s_msgs.insert(w.s_msgs.end(), msgs + msg_off[g], msgs + msg_off[g + 1]);
    w.s_moff.push_back(w.s_msgs.size());
  }
  c->stat_kagg[1] += nf; c->stat_kagg[2] += Ns;
  const KaCall B{w.sub.idx.data(), w.s_sigs.data(), w.sub.off.data(), w.s_msgs.data(), w.s_moff.data(), nf, dst, dst_len, wire};
  TRY(ka_attempt(c, k, B, true));
  w.s_out.resize(sb * nf); w.s_rows.resize(rb * nf); w.h_gbits.assign((nf + 7) / 8, 0);
  HIPCHK(c, hipMemcpyAsync(w.s_out.data(), d_out.p, sb * nf, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(w.s_rows.data(), w.rows.p, rb * nf, hipMemcpyDeviceToHost, c->stream));
  TRY(download(c, w.h_gbits.data(), w.gbits.p, (nf + 7) / 8));
  for (size_t j = 0; j < nf; ++j) {
    const size_t g = w.fail[j];
    if (!((w.h_gbits[j >> 3] >> (j & 7)) & 1)) { ++c->stat_kagg[3]; continue; }
    status[g] = 0;
    std::memcpy(out_sigs + sb * g, w.s_out.data() + sb * j, sb);
    std::memcpy(out_sel + g * rb, w.s_rows.data() + rb * j, rb);
  }
  return 0;
}

int blsbn254_keyset_aggregate_checked_batch(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* idx, const uint8_t* sigs, const uint64_t* sig_off,
                                            const uint8_t* msgs, const uint64_t* msg_off, size_t n_groups, const uint8_t* dst, size_t dst_len,
                                            uint8_t* out_sigs, uint8_t* out_sel, uint8_t* status) {
  return ka_checked(c, k, idx, sigs, sig_off, msgs, msg_off, n_groups, dst, dst_len, out_sigs, out_sel, status, false);
}
int blsbn254_keyset_aggregate_checked_batch_compressed(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* idx, const uint8_t* sigs, const uint64_t* sig_off,
                                                       const uint8_t* msgs, const uint64_t* msg_off, size_t n_groups, const uint8_t* dst, size_t dst_len,
                                                       uint8_t* out_sigs, uint8_t* out_sel, uint8_t* status) {
  return ka_checked(c, k, idx, sigs, sig_off, msgs, msg_off, n_groups, dst, dst_len, out_sigs, out_sel, status, true);
}

int blsbn254_keyset_aggregate_stats(blsbn254_ctx* c, uint64_t out[4]) {
  if (!c || !out) return BLSBN254_E_ARG;
  for (int i = 0; i < 4; ++i) out[i] = c->stat_kagg[i];
  return 0;
}

}  // extern "C"
