// host_keyset_merge.hip -- checked merge of partial aggregates over a registered key set: from the partial aggregates an
// intermediate node of an aggregation tree receives for one message per group, each an aggregate signature with the bitmap of
// the keys in it, ONE merged (aggregate, bitmap) pair per group, with the bad contributions left out.  Host side of
// include/blsbn254.h; kernels in k_keyset_merge.hip, lane functions in keyset_merge.h, the argument walk and the repack in
// keyset_merge_plan.h; see host_common.h and DESIGN.md 6j.
//
// The two attempts, the signature sums and the groups' equation are host_keyset_checked.hip's.  This form's own: an entry is a
// contribution (row, signature), every signature inflated on upload when compressed; the selection (ck_select) is greedy, disjoint
// candidates in the order given, a wave per group, and leaves the merged rows (k_km_select); the caller gets used bits; the key
// sums come from the merged rows by ks_enqueue_sums_dev.  The fallback repacks EVERY candidate of a failing group and verifies each
// by the key sum of ITS row where the sub-call's rows already are on the device (ck_verify_contributions); those bits are the
// selection's mask.  c->gs.sum / c->gs.pk serve that verification first and the groups' equation after it: stream order keeps
// the two uses apart, and both are reserved for the larger use before the first kernel is enqueued.
#include "host_common.h"

extern "C" {

static const uint64_t KM_MAX_ROW_BYTES = (uint64_t)1 << 30; // rows of one call, together

namespace {
struct KmCall { CkArgs a; const uint8_t* rows; };                      // rows indexed by the offsets as given
}

// One attempt over the groups of A, enqueued: the signature sums' encodings into c->kmrg.out (A.a.wire: wout as well), the merged
// rows into c->kmrg.orows, the used / candidate bitmaps into c->kmrg.used / cand, the bits of the groups' equation into gbits.
static int km_attempt(blsbn254_ctx* c, const blsbn254_keyset* k, const KmCall& A, bool fallback) {
  KmWs& w = c->kmrg;
  const size_t ng = A.a.n_groups, rb = (k->n + 7) / 8;
  TRY(stage_group_offsets(c, w.goff, A.a.ent_off, ng));
  const size_t N = w.goff.h[ng];
  HIPCHK(c, w.rows.reserve(rb * (N ? N : 1)));
  if (N) TRY(upload(c, w.rows, A.rows + rb * A.a.ent_off[0], rb * N));
  TRY(ck_stage_sigs(c, w, A.a, N, true));
  TRY(ck_reserve_key_sums(c, fallback ? std::max(std::min(N, c->chunk), ng) : ng));
  uint32_t dl;
  TRY(stage_dst(c, A.a.dst, A.a.dst_len, &dl));
  size_t word_launches;
  if (fallback && N)
    TRY(ck_verify_contributions(c, w, A.a, N, dl, false, [&](size_t lo, size_t m) {
      return ks_enqueue_sums_dev(c, k, (const uint8_t*)w.rows.p + lo * rb, m, &word_launches);
    }));
  HIPCHK(c, w.orows.reserve(rb * ng));
  TRY(ck_select(c, w, ng, N, [&](size_t lo, size_t m) {
    return launch(c, c->stream, "km_select", grid_lanes(64 * m), k_km_select, (const uint8_t*)w.rows.p, (const uint8_t*)w.sig_ok.p,
                  fallback ? (const uint8_t*)w.vbits.p : (const uint8_t*)nullptr, (const uint32_t*)w.goff.d.p, (const uint32_t*)k->vwords.p, (uint32_t)k->n, lo, m,
                  (uint8_t*)w.flags.p, (uint8_t*)w.orows.p);
  }));
  return ck_tail(c, w, A.a, dl, [&] { return ks_enqueue_sums_dev(c, k, (const uint8_t*)w.orows.p, ng, &word_launches); });
}

// both forms of the entry point; wire: sigs and out_sigs hold 32 bytes per signature
static int km_checked(blsbn254_ctx* c, const blsbn254_keyset* k, const uint8_t* rows, const uint8_t* sigs, const uint64_t* con_off, const uint8_t* msgs,
                      const uint64_t* msg_off, size_t n_groups, const uint8_t* dst, size_t dst_len, uint8_t* out_sigs, uint8_t* out_sel, uint8_t* used,
                      uint8_t* status, bool wire) {
  const KmCall A{{sigs, con_off, msgs, msg_off, n_groups, dst, dst_len, wire}, rows};
  if (const int rc = ck_args(c, k, A.a, !out_sigs || !out_sel || !used || !status, !rows, false, "contribution")) return rc == CK_NOTHING ? 0 : rc;
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
  const size_t rb = (k->n + 7) / 8;
  KmCall B{};                                                          // the sub-call, once the repack has run
  return ck_two_attempts(c, w, A.a, ck_even_rows(w, n_groups, rb), {out_sigs, out_sel, used, status}, c->kmrg.stat,
    [&](bool fallback) { return km_attempt(c, k, fallback ? B : A, fallback); },
    [&](const std::vector<size_t>& fail) {
      km_repack(fail, rows, sigs, con_off, w.h_cand.data(), rb, w.sub, wire ? 32 : 64);
      B = {{w.sub.sigs.data(), w.sub.off.data(), w.s_msgs.data(), w.s_moff.data(), fail.size(), dst, dst_len, wire}, w.sub.rows.data()};
      return CkSub{w.sub.pos.size(), w.even_off.data(), w.sub.pos.data(), w.sub.off.data()};
    });
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

int blsbn254_keyset_merge_stats(blsbn254_ctx* c, uint64_t out[4]) { return COPY_STATS(c, kmrg.stat, 4, out); }

}  // extern "C"
