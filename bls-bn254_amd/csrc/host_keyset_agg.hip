// host_keyset_agg.hip -- checked signature aggregation over a registered key set: from the individual signatures of committee
// members on one message per group, the aggregate signature and the participation row that
// blsbn254_keyset_fast_aggregate_verify_batch consumes, with the bad signatures left out.  Host side of include/blsbn254.h;
// kernels in k_keyset_agg.hip, lane functions in keyset_agg.h, the argument walk and the repack in keyset_agg_plan.h; see
// host_common.h and DESIGN.md 6i.
//
// The two attempts, the signature sums and the groups' equation are host_keyset_checked.hip's.  This form's own: an entry is
// (key index, signature); the candidate bit of every entry and its signature as a point come from k_ka_scan, the groups' rows
// from those bits (k_ka_rows), the key sums from the rows by ks_enqueue_sums_dev; the fallback gathers every entry's key from
// the handle's encodings and verifies every signature on its own (ck_verify_entries), and its bits are the scan's mask.
//
// The wire-format form (blsbn254_keyset_aggregate_checked_batch_compressed): the optimistic attempt scans the
// 32-byte entries where they are uploaded (k_ka_scan_wire inflates its own entry; no 64 N buffer exists); the fallback inflates
// its repacked entries into w.sigs, because the per-signature verification reads the 64-byte form.
#include "host_common.h"

extern "C" {

namespace {
struct KaCall { CkArgs a; const uint32_t* idx; };                      // idx indexed by the offsets as given
}

// One attempt over the groups of A, enqueued: the signature sums' encodings into c->kagg.out (A.a.wire: wout as well), the rows
// into c->kagg.orows, the bits of the groups' equation into c->kagg.gbits.
static int ka_attempt(blsbn254_ctx* c, const blsbn254_keyset* k, const KaCall& A, bool fallback) {
  KaggWs& w = c->kagg;
  const size_t ng = A.a.n_groups, rb = (k->n + 7) / 8, W = (k->n + 31) / 32;
  TRY(stage_group_offsets(c, w.goff, A.a.ent_off, ng));
  const size_t N = w.goff.h[ng], N1 = N ? N : 1;
  const bool scan_wire = A.a.wire && !fallback;                        // the scan inflates: no 64-byte form of the entries
  HIPCHK(c, w.idx.reserve(4 * N1));
  if (N) TRY(upload(c, w.idx, A.idx + A.a.ent_off[0], 4 * N));
  TRY(ck_stage_sigs(c, w, A.a, N, !scan_wire));
  TRY(ck_reserve_key_sums(c, ng));
  uint32_t dl;
  TRY(stage_dst(c, A.a.dst, A.a.dst_len, &dl));
  if (fallback && N) TRY(ck_verify_entries(c, k, w, w.pks, (const uint32_t*)w.idx.p, A.a, N));
  HIPCHK(c, w.cand.reserve((N + 7) / 8 + 8)); HIPCHK(c, w.pts.reserve(27 * N1 * 4)); HIPCHK(c, w.orows.reserve(rb * ng));
  TRY(for_chunks(c, N, [&](size_t lo, size_t m) {
    if (scan_wire)
      return launch(c, c->stream, "ka_scan_wire", grid_lanes(m), k_ka_scan_wire, (const uint8_t*)k->valid.p, (const uint32_t*)w.idx.p, (const uint8_t*)w.wire.p,
                    (const uint8_t*)nullptr, m, (uint32_t)lo, N, (uint8_t*)w.cand.p, (int32_t*)w.pts.p);
    return launch(c, c->stream, "ka_scan", grid_lanes(m), k_ka_scan, (const uint8_t*)k->valid.p, (const uint32_t*)w.idx.p, (const uint8_t*)w.sigs.p,
                  fallback ? (const uint8_t*)w.vbits.p : (const uint8_t*)nullptr, m, (uint32_t)lo, N, (uint8_t*)w.cand.p, (int32_t*)w.pts.p);
  }));
  // (the candidate bitmap is complete: every launch of the scan is enqueued before the first row is built)
  TRY(for_chunks(c, ng * W, [&](size_t lo, size_t m) {
    return launch(c, c->stream, "ka_rows", grid_lanes(m), k_ka_rows, (const uint32_t*)w.idx.p, (const uint8_t*)w.cand.p, (const uint32_t*)w.goff.d.p, m, lo, (uint32_t)k->n,
                  (uint8_t*)w.orows.p);
  }));
  return ck_tail(c, w, A.a, dl, [&] { size_t word_launches; return ks_enqueue_sums_dev(c, k, (const uint8_t*)w.orows.p, ng, &word_launches); });
}

// both forms of the entry point; wire: sigs and out_sigs hold 32 bytes per signature
static int ka_checked(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* idx, const uint8_t* sigs, const uint64_t* sig_off, const uint8_t* msgs,
                      const uint64_t* msg_off, size_t n_groups, const uint8_t* dst, size_t dst_len, uint8_t* out_sigs, uint8_t* out_sel, uint8_t* status, bool wire) {
  const KaCall A{{sigs, sig_off, msgs, msg_off, n_groups, dst, dst_len, wire}, idx};
  if (const int rc = ck_args(c, k, A.a, !out_sigs || !out_sel || !status, !idx, false, "group")) return rc == CK_NOTHING ? 0 : rc;
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
  const size_t rb = (k->n + 7) / 8, sb = wire ? 32 : 64;
  KaCall B{};                                                          // the sub-call, once the repack has run
  return ck_two_attempts(c, w, A.a, ck_even_rows(w, n_groups, rb), {out_sigs, out_sel, nullptr, status}, c->kagg.stat,
    [&](bool fallback) { return ka_attempt(c, k, fallback ? B : A, fallback); },
    [&](const std::vector<size_t>& fail) {
      ka_repack(fail, idx, sig_off, out_sel, rb, w.sub);               // (the candidates read off the downloaded rows; s_msgs / s_moff are final)
      const size_t Ns = w.sub.idx.size();
      w.s_sigs.resize(sb * Ns);
      for (size_t i = 0; i < Ns; ++i) std::memcpy(w.s_sigs.data() + sb * i, sigs + sb * w.sub.pos[i], sb);
      B = {{w.s_sigs.data(), w.sub.off.data(), w.s_msgs.data(), w.s_moff.data(), fail.size(), dst, dst_len, wire}, w.sub.idx.data()};
      return CkSub{Ns, w.even_off.data(), nullptr, nullptr};
    });
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

int blsbn254_keyset_aggregate_stats(blsbn254_ctx* c, uint64_t out[4]) { return COPY_STATS(c, kagg.stat, 4, out); }

}  // extern "C"
