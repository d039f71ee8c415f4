// host_keyset_committee_merge.hip -- checked merge of partial aggregates PER COMMITTEE of a registered key set:
// host_keyset_merge.hip for the intermediate node whose partial aggregates arrive per committee.  A group names a committee of
// the handle's table and brings contributions (a row as wide as the COMMITTEE, an aggregate signature); out come one merged
// aggregate and one merged row as wide as the committee, which the read-side committee calls of host_keyset_committee.hip
// consume as they are.  Nothing is as wide as the registry.  Host side of include/blsbn254.h; the kernel in
// k_keyset_committee_merge.hip, lane functions in keyset_committee_merge.h, the argument walk, the ragged layout and the repack
// in keyset_committee_merge_plan.h; see host_common.h and DESIGN.md 6p.
//
// The two attempts, the signature sums and the groups' equation are host_keyset_checked.hip's.  What differs from
// host_keyset_merge.hip: the selection walks the group's ragged rows and leaves the merged rows at their sel_off positions
// (k_kcm_select); the key sums run by the committee path (kc_enqueue_call_dev); the fallback verifies each contribution as a
// one-row group of that path, and because a launch's plan lives in c->kcom each launch is settled before the next is planned.
#include "host_common.h"

extern "C" {

static const uint64_t KCM_MAX_ROW_BYTES = (uint64_t)1 << 30; // contribution rows of one call, together

namespace {
struct KcmCall { CkArgs a; const uint32_t* com; const uint8_t* rows; const uint64_t* row_off; const uint64_t* sel_off; };   // rows indexed by the offsets as given
}

// One attempt over the groups of A, enqueued: the signature sums' encodings into c->kcmrg.out (A.a.wire: wout as well), the
// merged rows into c->kcmrg.orows (row g at sel_off[g] - sel_off[0]), the used / candidate bitmaps into c->kcmrg.used / cand, the
// bits of the groups' equation into c->kcmrg.gbits.
static int kcm_attempt(blsbn254_ctx* c, const blsbn254_keyset* k, const KcmCall& A, bool fallback) {
  KcmWs& w = c->kcmrg;
  const size_t ng = A.a.n_groups;
  TRY(stage_group_offsets(c, w.goff, A.a.ent_off, ng));
  const size_t N = w.goff.h[ng];
  kcm_layout(A.row_off, A.sel_off, ng, w.h_rbase, w.h_roff);              // (ctx-owned: the arrays outlive the uploads)
  const size_t in_bytes = w.h_rbase[ng], out_bytes = w.h_roff[ng];
  TRY(upload(c, w.com, A.com, 4 * ng));
  TRY(upload(c, w.rbase, w.h_rbase.data(), 8 * (ng + 1))); TRY(upload(c, w.roff, w.h_roff.data(), 8 * (ng + 1)));
  HIPCHK(c, w.rows.reserve(in_bytes ? in_bytes : 1));
  if (N) TRY(upload(c, w.rows, A.rows + A.row_off[0], in_bytes));
  TRY(ck_stage_sigs(c, w, A.a, N, true));
  TRY(ck_reserve_key_sums(c, fallback ? std::max(std::min(N, c->chunk), ng) : ng));
  uint32_t dl;
  TRY(stage_dst(c, A.a.dst, A.a.dst_len, &dl));
  if (fallback && N) {
    // a contribution is a one-row group of its group's committee
    kcm_layout_contributions(k->cm.tab, A.com, A.a.ent_off, ng, w.h_ccom, w.h_coff);
    TRY(ck_verify_contributions(c, w, A.a, N, dl, true, [&](size_t lo, size_t m) {
      return kc_enqueue_call_dev(c, k, w.h_ccom.data() + lo, (const uint8_t*)w.rows.p + w.h_coff[lo], w.h_coff.data() + lo, m);
    }));
  }
  HIPCHK(c, w.orows.reserve(out_bytes ? out_bytes : 1));
  TRY(ck_select(c, w, ng, N, [&](size_t lo, size_t m) {
    return launch(c, c->stream, "kcm_select", grid_lanes(64 * m), k_kcm_select, (const uint8_t*)w.rows.p, (const uint8_t*)w.sig_ok.p,
                  fallback ? (const uint8_t*)w.vbits.p : (const uint8_t*)nullptr, (const uint32_t*)w.goff.d.p, (const uint32_t*)w.com.p, (const uint4*)k->cm.coms.p,
                  (const uint32_t*)k->cm.cvalid.p, (const uint64_t*)w.rbase.p, (const uint64_t*)w.roff.p, lo, m, (uint8_t*)w.flags.p, (uint8_t*)w.orows.p);
  }));
  return ck_tail(c, w, A.a, dl, [&] { return kc_enqueue_call_dev(c, k, A.com, (const uint8_t*)w.orows.p, A.sel_off, ng); });
}

// both forms of the entry point; wire: sigs and out_sigs hold 32 bytes per signature
static int kcm_checked(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* com, const uint8_t* rows, const uint64_t* row_off, const uint8_t* sigs,
                       const uint64_t* con_off, const uint8_t* msgs, const uint64_t* msg_off, const uint64_t* sel_off, size_t n_groups, const uint8_t* dst,
                       size_t dst_len, uint8_t* out_sigs, uint8_t* out_sel, uint8_t* used, uint8_t* status, bool wire) {
  const KcmCall A{{sigs, con_off, msgs, msg_off, n_groups, dst, dst_len, wire}, com, rows, row_off, sel_off};
  if (const int rc = ck_args(c, k, A.a, !com || !row_off || !sel_off || !out_sigs || !out_sel || !used || !status, !rows, true, "contribution"))
    return rc == CK_NOTHING ? 0 : rc;
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
  KcmCall B{};                                                         // the sub-call, once the repack has run
  return ck_two_attempts(c, w, A.a, sel_off, {out_sigs, out_sel, used, status}, c->kcmrg.stat,
    [&](bool fallback) { return kcm_attempt(c, k, fallback ? B : A, fallback); },
    [&](const std::vector<size_t>& fail) {
      kcm_repack(T, fail, com, rows, row_off, sigs, con_off, w.h_cand.data(), w.sub, wire ? 32 : 64);
      B = {{w.sub.sigs.data(), w.sub.off.data(), w.s_msgs.data(), w.s_moff.data(), fail.size(), dst, dst_len, wire}, w.sub.com.data(), w.sub.rows.data(),
           w.sub.row_off.data(), w.sub.sel_off.data()};
      return CkSub{w.sub.pos.size(), w.sub.sel_off.data(), w.sub.pos.data(), w.sub.off.data()};
    });
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

int blsbn254_keyset_committee_merge_stats(blsbn254_ctx* c, uint64_t out[4]) { return COPY_STATS(c, kcmrg.stat, 4, out); }

}  // extern "C"
