// host_keyset_committee_agg.hip -- checked signature aggregation PER COMMITTEE of a registered key set: host_keyset_agg.hip for
// the collector whose signatures arrive per committee.  A group names a committee of the handle's table and brings entries
// (position in the member list, signature); out come the aggregate and a row as wide as the COMMITTEE, which the read-side
// committee calls of host_keyset_committee.hip consume as they are.  Nothing is as wide as the registry.  Host side of
// include/blsbn254.h; kernels in k_keyset_committee_agg.hip, lane functions in keyset_committee_agg.h, the argument walk, the
// ragged layout and the repack in keyset_committee_agg_plan.h; see host_common.h and DESIGN.md 6o.
//
// The two attempts, the signature sums and the groups' equation are host_keyset_checked.hip's.  What differs from
// host_keyset_agg.hip: the scan tests the validity bit of the entry's position in the committee's words, no member index
// (k_kca_scan, k_kca_scan_wire); the rows are ragged, row g at sel_off[g] - sel_off[0] (k_kca_rows); the key sums run by the
// committee path (kc_enqueue_call_dev); the fallback resolves every entry's registry index from the member list (k_kca_resolve)
// before its key is gathered by it.
#include "host_common.h"

extern "C" {

namespace {
struct KcaCall { CkArgs a; const uint32_t* com; const uint32_t* pos; const uint64_t* sel_off; };   // pos indexed by the offsets as given
}

// One attempt over the groups of A, enqueued: the signature sums' encodings into c->kcagg.out (A.a.wire: wout as well), the rows
// into c->kcagg.orows (row g at sel_off[g] - sel_off[0]), the bits of the groups' equation into c->kcagg.gbits.
static int kca_attempt(blsbn254_ctx* c, const blsbn254_keyset* k, const KcaCall& A, bool fallback) {
  KcaWs& w = c->kcagg;
  const size_t ng = A.a.n_groups;
  TRY(stage_group_offsets(c, w.goff, A.a.ent_off, ng));
  const size_t N = w.goff.h[ng], N1 = N ? N : 1;
  kca_layout(k->cm.tab, A.com, A.sel_off, ng, w.h_wpre, w.h_roff);     // (ctx-owned: the arrays outlive the uploads)
  const size_t n_words = w.h_wpre[ng], row_bytes = w.h_roff[ng];
  TRY(upload(c, w.com, A.com, 4 * ng));
  TRY(upload(c, w.wpre, w.h_wpre.data(), 8 * (ng + 1))); TRY(upload(c, w.roff, w.h_roff.data(), 8 * (ng + 1)));
  const bool scan_wire = A.a.wire && !fallback;                        // the scan inflates: no 64-byte form of the entries
  HIPCHK(c, w.pos.reserve(4 * N1));
  if (N) TRY(upload(c, w.pos, A.pos + A.a.ent_off[0], 4 * N));
  TRY(ck_stage_sigs(c, w, A.a, N, !scan_wire));
  TRY(ck_reserve_key_sums(c, ng));
  uint32_t dl;
  TRY(stage_dst(c, A.a.dst, A.a.dst_len, &dl));
  const uint32_t* goff = (const uint32_t*)w.goff.d.p;
  const uint4* coms = (const uint4*)k->cm.coms.p;
  const uint32_t* com = (const uint32_t*)w.com.p;
  if (fallback && N) {
    HIPCHK(c, w.ridx.reserve(4 * N));
    TRY(for_chunks(c, N, [&](size_t lo, size_t m) {
      return launch(c, c->stream, "kca_resolve", grid_lanes(m), k_kca_resolve, (const uint32_t*)k->cm.members.p, coms, com, goff, (uint32_t)ng, (const uint32_t*)w.pos.p, m,
                    (uint32_t)lo, (uint32_t*)w.ridx.p);
    }));
    TRY(ck_verify_entries(c, k, w, w.pks, (const uint32_t*)w.ridx.p, A.a, N));
  }
  HIPCHK(c, w.cand.reserve((N + 7) / 8 + 8)); HIPCHK(c, w.pts.reserve(27 * N1 * 4)); HIPCHK(c, w.orows.reserve(row_bytes));
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
                  (const uint64_t*)w.roff.p, coms, com, (uint32_t)ng, m, (uint64_t)lo, (uint8_t*)w.orows.p);
  }));
  return ck_tail(c, w, A.a, dl, [&] { return kc_enqueue_call_dev(c, k, A.com, (const uint8_t*)w.orows.p, A.sel_off, ng); });
}

// both forms of the entry point; wire: sigs and out_sigs hold 32 bytes per signature
static int kca_checked(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* com, const uint32_t* pos, const uint8_t* sigs, const uint64_t* sig_off,
                       const uint8_t* msgs, const uint64_t* msg_off, const uint64_t* sel_off, size_t n_groups, const uint8_t* dst, size_t dst_len, uint8_t* out_sigs,
                       uint8_t* out_sel, uint8_t* status, bool wire) {
  const KcaCall A{{sigs, sig_off, msgs, msg_off, n_groups, dst, dst_len, wire}, com, pos, sel_off};
  if (const int rc = ck_args(c, k, A.a, !com || !sel_off || !out_sigs || !out_sel || !status, !pos, true, "group")) return rc == CK_NOTHING ? 0 : rc;
  if (check_offsets(sel_off, n_groups)) { c->last_error = "row offsets decrease"; return BLSBN254_E_ARG; }
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
  const size_t sb = wire ? 32 : 64;
  KcaCall B{};                                                         // the sub-call, once the repack has run
  return ck_two_attempts(c, w, A.a, sel_off, {out_sigs, out_sel, nullptr, status}, c->kcagg.stat,
    [&](bool fallback) { return kca_attempt(c, k, fallback ? B : A, fallback); },
    [&](const std::vector<size_t>& fail) {
      kca_repack(fail, com, pos, sig_off, sel_off, out_sel, w.sub);    // (the candidates read off the downloaded rows)
      const size_t Ns = w.sub.pos.size();
      w.s_sigs.resize(sb * Ns);
      for (size_t i = 0; i < Ns; ++i) std::memcpy(w.s_sigs.data() + sb * i, sigs + sb * w.sub.src[i], sb);
      B = {{w.s_sigs.data(), w.sub.off.data(), w.s_msgs.data(), w.s_moff.data(), fail.size(), dst, dst_len, wire}, w.sub.com.data(), w.sub.pos.data(),
           w.sub.sel_off.data()};
      return CkSub{Ns, w.sub.sel_off.data(), nullptr, nullptr};
    });
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

int blsbn254_keyset_committee_aggregate_stats(blsbn254_ctx* c, uint64_t out[4]) { return COPY_STATS(c, kcagg.stat, 4, out); }

}  // extern "C"
