// host_threshold_deal.hip -- the dealing side of the threshold scheme over ragged groups: key shares f_g(id) in Fr, their
// public keys sum_j [id^j] C_j from a group's Feldman commitments, and the check of partial signatures against those keys.
// Host side of include/blsbn254.h; kernels in k_threshold_deal.hip (one lane per SHARE over all groups of a call); see
// host_common.h.
//
// Coefficients / commitments are uploaded and decoded ONCE per call (k_fr_coef_decode; k_g2_load + k_g2_check over all T of
// them -- a launch may span MAX_LANES elements, which is the limit of T).  The shares run in launches of at most ctx->chunk
// lanes; a lane depends on no other share, so a launch may end anywhere: ids decoded (k_fr_decode), Horner per lane into the
// call's workspace of shares (Montgomery limbs / homogeneous points).  After the last launch the marks the lanes left and the
// validity bytes of the coefficients become statuses (k_td_finish), the shares are encoded -- those of a marked group as
// zero bytes / the identity -- again by chunks, then ONE download and synchronisation.
// The check of dealt key shares (blsbn254_threshold_verify_key_shares_batch) runs the G2 evaluation up to and including
// k_td_finish, leaves the key shares homogeneous in the workspace and compares them there (k_threshold_keycheck.hip).
#include "host_common.h"
#include "threshold_keycheck.h"   // TD_MAX_BITS, the bits of a group's mark word, the shape of the generator table

extern "C" {

// the largest bit length among the m ids at `ids` (32 B big-endian each), at least 1 and capped at TD_MAX_BITS: ids that the
// kernels will reject (>= r) are counted like any other
static int td_id_bits(const uint8_t* ids, size_t m) {
  int best = 1;
  for (size_t i = 0; i < m; ++i) {
    for (int w = 0; w < 4; ++w) {                                    // 64-bit words, most significant first
      uint64_t v;
      std::memcpy(&v, ids + 32 * i + 8 * w, 8);
      if (!v) continue;
      best = std::max(best, 64 * (3 - w) + 64 - __builtin_clzll(__builtin_bswap64(v)));
      break;
    }
  }
  return std::min(best, TD_MAX_BITS);
}
int td_stage_commitments(blsbn254_ctx* c, const uint8_t* commitments, const uint64_t* coef_off, size_t n_groups) {
  TdlWs& w = c->tdl;
  const size_t T = (size_t)(coef_off[n_groups] - coef_off[0]), T1 = T ? T : 1;
  HIPCHK(c, w.c_ws.reserve(54 * T1 * 4)); HIPCHK(c, w.c_ok.reserve(T1)); HIPCHK(c, w.c_sub.reserve(T1)); HIPCHK(c, w.coef.reserve(128 * T1));
  if (!T) return 0;
  TRY(upload(c, w.coef, commitments + 128 * coef_off[0], 128 * T));
  TRY(launch(c, c->stream, "g2_load", grid_lanes(T), k_g2_load, (const uint8_t*)w.coef.p, T, (int32_t*)w.c_ws.p, (uint8_t*)w.c_ok.p));
  return launch(c, c->stream, "g2_check", grid_lanes(T), k_g2_check, (const uint8_t*)w.coef.p, T, (uint8_t*)w.c_sub.p, (uint8_t*)nullptr);
}
int td_args(blsbn254_ctx* c, const void* coefs, const uint64_t* coef_off, const uint8_t* ids, const uint64_t* id_off, size_t n_groups, const void* out, const void* status) {
  if (!coef_off || !id_off || !status) return BLSBN254_E_ARG;
  if (check_offsets(coef_off, n_groups) || check_offsets(id_off, n_groups)) { c->last_error = "group offsets decrease"; return BLSBN254_E_ARG; }
  const size_t N = (size_t)(id_off[n_groups] - id_off[0]), T = (size_t)(coef_off[n_groups] - coef_off[0]);
  if ((N && (!ids || !out)) || (T && !coefs)) return BLSBN254_E_ARG;
  CHECK_LANES(c, N);
  CHECK_LANES(c, T);
  CHECK_LANES(c, n_groups);
  return 0;
}
// the arguments a call with one message per group adds to td_args (checked after it)
int td_msg_args(blsbn254_ctx* c, const uint8_t* partial_sigs, const uint64_t* id_off, const uint8_t* msgs, const uint64_t* msg_off, size_t n_groups,
                const uint8_t* dst, size_t dst_len) {
  if (!msg_off || (dst_len && !dst)) return BLSBN254_E_ARG;
  if (check_offsets(msg_off, n_groups)) { c->last_error = "message offsets decrease"; return BLSBN254_E_ARG; }
  if (id_off[n_groups] != id_off[0] && !partial_sigs) return BLSBN254_E_ARG;
  if (!msgs && msg_off[n_groups] != msg_off[0]) return BLSBN254_E_ARG;
  return 0;
}

// The G2 evaluation for all groups up to and including k_td_finish: the N key shares homogeneous in c->tdl.r_ws (limb-major,
// stride N), the groups' marks complete in c->tdl.gstat, the per-group statuses in c->tdl.st.  Enqueued.
static int td_g2_eval_enqueue(blsbn254_ctx* c, const uint8_t* commitments, const uint64_t* coef_off, const uint8_t* ids, const uint64_t* id_off, size_t n_groups) {
  TdlWs& w = c->tdl;
  TRY(stage_group_offsets(c, w.goff, id_off, n_groups)); TRY(stage_group_offsets(c, w.coff, coef_off, n_groups));
  HIPCHK(c, w.gstat.reserve(4 * n_groups)); HIPCHK(c, w.st.reserve(n_groups));
  HIPCHK(c, hipMemsetAsync(w.gstat.p, 0, 4 * n_groups, c->stream));
  const size_t N = w.goff.h[n_groups], T = w.coff.h[n_groups];
  const uint32_t* goff = (const uint32_t*)w.goff.d.p; const uint32_t* coff = (const uint32_t*)w.coff.d.p;
  uint32_t* gstat = (uint32_t*)w.gstat.p;
  TRY(td_stage_commitments(c, commitments, coef_off, n_groups));
  if (N) {
    const size_t m1 = std::min(N, c->chunk);
    HIPCHK(c, c->th.x.reserve(9 * m1 * 4)); HIPCHK(c, c->status.reserve(m1)); HIPCHK(c, w.r_ws.reserve(54 * N * 4));
    TRY(upload(c, w.ids, ids + 32 * id_off[0], 32 * N));
    TRY(for_chunks(c, N, [&](size_t lo, size_t m) {
      const int nbits = td_id_bits(ids + 32 * (id_off[0] + lo), m);
      ++c->tdl.stat[0]; c->tdl.stat[1] += m; c->tdl.stat[3] = (uint64_t)nbits;
      TRY(launch(c, c->stream, "fr_decode", grid_lanes(m), k_fr_decode, (const uint8_t*)w.ids.p + 32 * lo, m, (int32_t*)c->th.x.p, (uint8_t*)c->status.p));
      return launch(c, c->stream, "g2_poly_eval", grid_lanes(m), k_g2_poly_eval, (const int32_t*)c->th.x.p, (const uint8_t*)c->status.p, m, (uint32_t)lo, goff, coff,
                    (uint32_t)n_groups, (const int32_t*)w.c_ws.p, T, nbits, (int32_t*)w.r_ws.p, N, gstat);
    }));
  }
  return launch(c, c->stream, "td_finish", grid_lanes(n_groups), k_td_finish, gstat, n_groups, coff, (const uint8_t*)w.c_ok.p, (const uint8_t*)w.c_sub.p, (uint32_t)TD_MARK_POINT,
                (uint8_t*)w.st.p);
}
// The device part of the G2 evaluation for all groups: the N public key shares in wire format into d_pks (device), the
// per-group statuses into c->tdl.st.  Everything is enqueued; the caller downloads and synchronises.
static int td_g2_enqueue(blsbn254_ctx* c, const uint8_t* commitments, const uint64_t* coef_off, const uint8_t* ids, const uint64_t* id_off, size_t n_groups, uint8_t* d_pks) {
  TRY(td_g2_eval_enqueue(c, commitments, coef_off, ids, id_off, n_groups));
  TdlWs& w = c->tdl;
  const size_t N = w.goff.h[n_groups];
  return for_chunks(c, N, [&](size_t lo, size_t m) {
    return launch(c, c->stream, "td_g2_encode", grid_lanes(m), k_td_g2_encode, (const int32_t*)w.r_ws.p, N, m, (uint32_t)lo, (const uint32_t*)w.goff.d.p, (uint32_t)n_groups,
                  (const uint32_t*)w.gstat.p, d_pks + 128 * lo);
  });
}

int blsbn254_fr_poly_eval_batch(blsbn254_ctx* c, const uint8_t* coeffs, const uint64_t* coef_off, const uint8_t* ids, const uint64_t* id_off, size_t n_groups,
                                uint8_t* out, uint8_t* status) {
  if (!c) return BLSBN254_E_ARG;
  if (n_groups == 0) return 0;
  int rc = td_args(c, coeffs, coef_off, ids, id_off, n_groups, out, status);
  if (rc) return rc;
  ENTER(c);
  TdlWs& w = c->tdl;
  TRY(stage_group_offsets(c, w.goff, id_off, n_groups)); TRY(stage_group_offsets(c, w.coff, coef_off, n_groups));
  HIPCHK(c, w.gstat.reserve(4 * n_groups)); HIPCHK(c, w.st.reserve(n_groups));
  HIPCHK(c, hipMemsetAsync(w.gstat.p, 0, 4 * n_groups, c->stream));
  const size_t N = w.goff.h[n_groups], T = w.coff.h[n_groups], T1 = T ? T : 1;
  const uint32_t* goff = (const uint32_t*)w.goff.d.p; const uint32_t* coff = (const uint32_t*)w.coff.d.p;
  uint32_t* gstat = (uint32_t*)w.gstat.p;
  HIPCHK(c, w.cf_ws.reserve(9 * T1 * 4)); HIPCHK(c, w.c_ok.reserve(T1));
  if (T) {
    TRY(upload(c, w.coef, coeffs + 32 * coef_off[0], 32 * T));
    TRY(launch(c, c->stream, "fr_coef_decode", grid_lanes(T), k_fr_coef_decode, (const uint8_t*)w.coef.p, T, (int32_t*)w.cf_ws.p, (uint8_t*)w.c_ok.p));
  }
  if (N) {
    const size_t m1 = std::min(N, c->chunk);
    HIPCHK(c, c->th.x.reserve(9 * m1 * 4)); HIPCHK(c, c->status.reserve(m1)); HIPCHK(c, w.r_ws.reserve(9 * N * 4)); HIPCHK(c, c->out.reserve(32 * N));
    TRY(upload(c, w.ids, ids + 32 * id_off[0], 32 * N));
    TRY(for_chunks(c, N, [&](size_t lo, size_t m) {
      c->tdl.stat[2] += m;
      TRY(launch(c, c->stream, "fr_decode", grid_lanes(m), k_fr_decode, (const uint8_t*)w.ids.p + 32 * lo, m, (int32_t*)c->th.x.p, (uint8_t*)c->status.p));
      return launch(c, c->stream, "fr_poly_eval", grid_lanes(m), k_fr_poly_eval, (const int32_t*)c->th.x.p, (const uint8_t*)c->status.p, m, (uint32_t)lo, goff, coff,
                    (uint32_t)n_groups, (const int32_t*)w.cf_ws.p, T, (int32_t*)w.r_ws.p, N, gstat);
    }));
  }
  TRY(launch(c, c->stream, "td_finish", grid_lanes(n_groups), k_td_finish, gstat, n_groups, coff, (const uint8_t*)w.c_ok.p, (const uint8_t*)nullptr, (uint32_t)TD_MARK_SCALAR,
             (uint8_t*)w.st.p));
  if (N) {
    TRY(for_chunks(c, N, [&](size_t lo, size_t m) {
      return launch(c, c->stream, "td_fr_encode", grid_lanes(m), k_td_fr_encode, (const int32_t*)w.r_ws.p, N, m, (uint32_t)lo, goff, (uint32_t)n_groups, (const uint32_t*)gstat,
                    (uint8_t*)c->out.p + 32 * lo);
    }));
    HIPCHK(c, hipMemcpyAsync(out, c->out.p, 32 * N, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipMemcpyAsync(status, w.st.p, n_groups, hipMemcpyDeviceToHost, c->stream));
  // the staged coefficients, their decoded form and both device copies of the shares do not outlive the call
  if (T) { HIPCHK(c, hipMemsetAsync(w.coef.p, 0, 32 * T, c->stream)); HIPCHK(c, hipMemsetAsync(w.cf_ws.p, 0, 9 * T * 4, c->stream)); }
  if (N) { HIPCHK(c, hipMemsetAsync(w.r_ws.p, 0, 9 * N * 4, c->stream)); HIPCHK(c, hipMemsetAsync(c->out.p, 0, 32 * N, c->stream)); }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int blsbn254_g2_poly_eval_batch(blsbn254_ctx* c, const uint8_t* commitments, const uint64_t* coef_off, const uint8_t* ids, const uint64_t* id_off, size_t n_groups,
                                uint8_t* out_pks, uint8_t* status) {
  if (!c) return BLSBN254_E_ARG;
  if (n_groups == 0) return 0;
  int rc = td_args(c, commitments, coef_off, ids, id_off, n_groups, out_pks, status);
  if (rc) return rc;
  ENTER(c);
  const size_t N = (size_t)(id_off[n_groups] - id_off[0]);
  HIPCHK(c, c->tdl.pks.reserve(128 * (N ? N : 1)));
  TRY(td_g2_enqueue(c, commitments, coef_off, ids, id_off, n_groups, (uint8_t*)c->tdl.pks.p));
  if (N) HIPCHK(c, hipMemcpyAsync(out_pks, c->tdl.pks.p, 128 * N, hipMemcpyDeviceToHost, c->stream));
  return download(c, status, c->tdl.st.p, n_groups);
}

// The device part of the check of partial signatures (arguments already checked): the key shares evaluated into c->tdl.pks,
// the N bits into c->bitmap, the groups' statuses into c->tdl.st.  Enqueued; the caller downloads and synchronises.
int td_verify_shares_enqueue(blsbn254_ctx* c, const uint8_t* commitments, const uint64_t* coef_off, const uint8_t* ids, const uint8_t* partial_sigs,
                             const uint64_t* id_off, const uint8_t* msgs, const uint64_t* msg_off, size_t n_groups, const uint8_t* dst, size_t dst_len) {
  const size_t N = (size_t)(id_off[n_groups] - id_off[0]);
  TdlWs& w = c->tdl;
  HIPCHK(c, w.pks.reserve(128 * (N ? N : 1)));
  TRY(td_g2_enqueue(c, commitments, coef_off, ids, id_off, n_groups, (uint8_t*)w.pks.p));
  if (!N) return 0;
  // the verify pipeline takes one message per tuple: the group's message once per share (ctx-owned: outlives the upload)
  w.h_msgs.clear(); w.h_moff.resize(N + 1);
  size_t i = 0;
  w.h_moff[0] = 0;
  for (size_t g = 0; g < n_groups; ++g) {
    const size_t len = (size_t)(msg_off[g + 1] - msg_off[g]);
    for (uint64_t s = id_off[g]; s < id_off[g + 1]; ++s, ++i) {
      if (len) w.h_msgs.insert(w.h_msgs.end(), msgs + msg_off[g], msgs + msg_off[g + 1]);
      w.h_moff[i + 1] = w.h_moff[i] + len;
    }
  }
  TRY(stage_msgs(c, w.h_msgs.data(), w.h_moff.data(), N));
  HIPCHK(c, c->bitmap.reserve((N + 7) / 8 + 8));
  TRY(upload(c, c->in_b, partial_sigs + 64 * id_off[0], 64 * N));
  // the public key shares never leave the device; the counting path, so that nothing is left pending and the bitmap is
  // final behind this call on the stream
  return blsbn254_internal_verify_batch_dev_sync(c, (const uint8_t*)w.pks.p, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, (const uint8_t*)c->in_b.p, N, dst, dst_len,
                                                 (uint8_t*)c->bitmap.p);
}

int blsbn254_threshold_verify_shares_batch(blsbn254_ctx* c, const uint8_t* commitments, const uint64_t* coef_off, const uint8_t* ids, const uint8_t* partial_sigs,
                                           const uint64_t* id_off, const uint8_t* msgs, const uint64_t* msg_off, size_t n_groups, const uint8_t* dst, size_t dst_len,
                                           uint8_t* valid_bitmap, uint8_t* status) {
  if (!c) return BLSBN254_E_ARG;
  if (n_groups == 0) return 0;
  int rc = td_args(c, commitments, coef_off, ids, id_off, n_groups, valid_bitmap, status);
  if (rc) return rc;
  TRY(td_msg_args(c, partial_sigs, id_off, msgs, msg_off, n_groups, dst, dst_len));
  const size_t N = (size_t)(id_off[n_groups] - id_off[0]);
  ENTER(c);
  TRY(td_verify_shares_enqueue(c, commitments, coef_off, ids, partial_sigs, id_off, msgs, msg_off, n_groups, dst, dst_len));
  if (N) HIPCHK(c, hipMemcpyAsync(valid_bitmap, c->bitmap.p, (N + 7) / 8, hipMemcpyDeviceToHost, c->stream));
  return download(c, status, c->tdl.st.p, n_groups);
}

// the table of the generator's multiples, built on the device at the first call that needs it and kept for the context's life
static int kc_table(blsbn254_ctx* c) {
  if (c->kchk.stat[2]) return 0;
  HIPCHK(c, c->kchk.tab.reserve(KC_TABLE_LIMBS * 4));
  TRY(launch(c, c->stream, "g2gen_table", Shape{dim3((KC_WINDOWS + 63) / 64), dim3(64)}, k_g2gen_table, (int32_t*)c->kchk.tab.p));
  ++c->kchk.stat[2];
  return 0;
}

int blsbn254_threshold_verify_key_shares_batch(blsbn254_ctx* c, const uint8_t* commitments, const uint64_t* coef_off, const uint8_t* ids, const uint8_t* shares,
                                               const uint64_t* id_off, size_t n_groups, uint8_t* valid_bitmap, uint8_t* status) {
  if (!c) return BLSBN254_E_ARG;
  if (n_groups == 0) return 0;
  int rc = td_args(c, commitments, coef_off, ids, id_off, n_groups, valid_bitmap, status);
  if (rc) return rc;
  const size_t N = (size_t)(id_off[n_groups] - id_off[0]);
  if (N && !shares) return BLSBN254_E_ARG;
  ENTER(c);
  TdlWs& w = c->tdl;
  if (N) {
    TRY(kc_table(c));
    HIPCHK(c, w.share_ok.reserve(N)); HIPCHK(c, c->bitmap.reserve((N + 7) / 8));
    TRY(upload(c, w.shares, shares + 32 * id_off[0], 32 * N));
  }
  TRY(td_g2_eval_enqueue(c, commitments, coef_off, ids, id_off, n_groups));
  if (N) {
    TRY(for_chunks(c, N, [&](size_t lo, size_t m) {
      ++c->kchk.stat[0]; c->kchk.stat[1] += m;
      return launch(c, c->stream, "td_key_check", grid_lanes(m), k_td_key_check, (const uint8_t*)w.shares.p, m, (uint32_t)lo, (const int32_t*)c->kchk.tab.p,
                    (const int32_t*)w.r_ws.p, N, (uint8_t*)w.share_ok.p);
    }));
    // a share's bit needs its group's marks, complete only behind the last launch and k_td_finish
    TRY(launch(c, c->stream, "td_key_bits", grid_lanes((N + 7) / 8), k_td_key_bits, (const uint8_t*)w.share_ok.p, N, (const uint32_t*)w.goff.d.p, (uint32_t)n_groups,
               (const uint32_t*)w.gstat.p, (uint8_t*)c->bitmap.p));
    HIPCHK(c, hipMemcpyAsync(valid_bitmap, c->bitmap.p, (N + 7) / 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemsetAsync(w.shares.p, 0, 32 * N, c->stream));      // the staged shares do not outlive the call
  }
  return download(c, status, w.st.p, n_groups);
}

int blsbn254_threshold_key_check_stats(blsbn254_ctx* c, uint64_t out[4]) {
  TRY(COPY_STATS(c, kchk.stat, 3, out));
  out[3] = (uint64_t)KC_WINDOW_BITS;
  return 0;
}

int blsbn254_threshold_deal_stats(blsbn254_ctx* c, uint64_t out[4]) { return COPY_STATS(c, tdl.stat, 4, out); }

}  // extern "C"
