// host_keyset_weight.hip -- stake weights on a registered key set and FastAggregateVerify with a quorum: per group the sums of
// the selected keys' stake columns, and a verify call that weighs first and sums and pairs only the groups that reach the
// quorum.  Host side of include/blsbn254.h; kernels in k_keyset_weight.hip, lane functions in keyset_weight.h, the column check,
// the quorum rule and the repack in keyset_weight_plan.h; see host_common.h and DESIGN.md 6k.  (The registration with proofs of
// possession is blsbn254_keyset_create_checked in host_keyset.hip, beside the registration it extends.)
//
// blsbn254_keyset_quorum_verify_batch: the rows are staged once (c->kset.sel), weighed, and the weights read back -- the call's
// one extra synchronisation.  Every group reaches quorum: the staged rows go to ks_verify_rows as they are.  Some do: the host
// repacks the reaching groups' rows, messages and signatures (kw_repack) and ks_verify_rows runs on that sub-call, its bits
// scattered into the call's bitmap.  None does: nothing more is launched.  A group below quorum is neither summed nor paired.
#include "host_common.h"

extern "C" {

// the weights of n_groups rows ALREADY ON THE DEVICE into d_out (n_groups x n_cols), enqueued: a wave per group, launches of at
// most c->chunk / 64 groups
static int kw_enqueue(blsbn254_ctx* c, const blsbn254_keyset* k, const uint8_t* d_rows, size_t n_groups, uint64_t* d_out, size_t* launches) {
  const size_t Gl = kw_launch_groups(c->chunk);
  *launches = 0;
  for (size_t lo = 0; lo < n_groups; lo += Gl, ++*launches) {
    const size_t m = std::min(Gl, n_groups - lo);
    TRY(launch(c, c->stream, "ks_weight", grid_lanes(64 * m), k_ks_weight, d_rows, (const uint32_t*)k->vwords.p, (const uint64_t*)k->weff.p, (uint32_t)k->n, (uint32_t)k->n_cols, lo, m, d_out));
  }
  return 0;
}
static int kw_handle(blsbn254_ctx* c, const blsbn254_keyset* k) {
  if (!k || k->ctx != c) return BLSBN254_E_ARG;
  if (k->n_cols == 0) { c->last_error = "the key set has no weights (blsbn254_keyset_set_weights)"; return BLSBN254_E_ARG; }
  return 0;
}

int blsbn254_keyset_set_weights(blsbn254_ctx* c, blsbn254_keyset* k, const uint64_t* weights, size_t n_cols) {
  if (!c || !k || k->ctx != c || !weights) return BLSBN254_E_ARG;
  if (n_cols == 0 || n_cols > BLSBN254_KS_MAX_COLS) { c->last_error = "1 to 8 weight columns"; return BLSBN254_E_ARG; }
  const int bad = kw_overflowing_column(weights, k->n, n_cols);
  if (bad >= 0) { c->last_error = "the sum of weight column " + std::to_string(bad) + " does not fit 64 bits"; return BLSBN254_E_ARG; }
  ENTER(c);
  KwWs& w = c->kw;
  const size_t n = k->n, rb = (n + 7) / 8;
  // every enqueued reader of the old table is done before it is replaced (the calls that read it end synchronised; this wait
  // covers a caller that mixes contexts' streams by hand)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  k->n_cols = 0;                                           // no table while the new one is being made: a failure below leaves none
  HIPCHK(c, w.out.reserve(8 * BLSBN254_KS_MAX_COLS));
  kw_key_major(weights, n, n_cols, w.h_tab);               // ctx-owned: outlives the upload
  TRY(upload(c, k->weff, w.h_tab.data(), 8 * n * n_cols));
  // the totals: the weights of the row that selects every key (ctx-owned: outlives the upload)
  w.h_ones.assign(rb, 0xff);
  if (n & 7) w.h_ones[rb - 1] = (uint8_t)(0xffu >> (8 - (n & 7)));
  TRY(upload(c, c->kset.sel, w.h_ones.data(), rb));
  k->n_cols = n_cols;
  size_t launches;
  int rc = kw_enqueue(c, k, (const uint8_t*)c->kset.sel.p, 1, (uint64_t*)w.out.p, &launches);
  if (!rc) rc = download(c, k->wtotal, w.out.p, 8 * n_cols);
  if (rc) { (void)hipStreamSynchronize(c->stream); k->n_cols = 0; return rc; }
  ++c->kw.stat[3];
  return 0;
}

int blsbn254_keyset_total_weight(blsbn254_ctx* c, const blsbn254_keyset* k, uint64_t* out) {
  if (!c || !out) return BLSBN254_E_ARG;
  TRY(kw_handle(c, k));
  std::memcpy(out, k->wtotal, 8 * k->n_cols);
  return 0;
}

int blsbn254_keyset_weight_batch(blsbn254_ctx* c, const blsbn254_keyset* k, const uint8_t* sel, size_t n_groups, uint64_t* out) {
  if (!c || (n_groups && (!sel || !out))) return BLSBN254_E_ARG;
  TRY(kw_handle(c, k));
  if (n_groups == 0) return 0;
  TRY(ks_args(c, k, sel, n_groups));
  ENTER(c);
  KwWs& w = c->kw;
  HIPCHK(c, w.out.reserve(8 * k->n_cols * n_groups));
  TRY(upload(c, c->kset.sel, sel, (k->n + 7) / 8 * n_groups));
  size_t launches;
  TRY(kw_enqueue(c, k, (const uint8_t*)c->kset.sel.p, n_groups, (uint64_t*)w.out.p, &launches));
  TRY(download(c, out, w.out.p, 8 * k->n_cols * n_groups));
  c->kw.stat[0] += n_groups; c->kw.stat[2] += launches;
  return 0;
}

int blsbn254_keyset_quorum_verify_batch(blsbn254_ctx* c, const blsbn254_keyset* k, const uint8_t* sel, const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs,
                                        size_t n_groups, const uint8_t* dst, size_t dst_len, const uint64_t* min_weight, uint64_t* weights_out,
                                        uint8_t* valid_bitmap) {
  if (!c || !off || !min_weight || (n_groups && (!sel || !sigs || !valid_bitmap || !weights_out)) || (dst_len && !dst)) return BLSBN254_E_ARG;
  TRY(kw_handle(c, k));
  if (n_groups == 0) return 0;
  TRY(ks_args(c, k, sel, n_groups));
  if (check_offsets(off, n_groups)) { c->last_error = "message offsets decrease"; return BLSBN254_E_ARG; }
  if (!msgs && off[n_groups] != off[0]) { c->last_error = "a NULL argument"; return BLSBN254_E_ARG; }
  ENTER(c);
  KwWs& w = c->kw;
  const size_t rb = (k->n + 7) / 8, nb = (n_groups + 7) / 8, nc = k->n_cols;
  HIPCHK(c, w.out.reserve(8 * nc * n_groups));
  TRY(upload(c, c->kset.sel, sel, rb * n_groups));
  size_t launches;
  TRY(kw_enqueue(c, k, (const uint8_t*)c->kset.sel.p, n_groups, (uint64_t*)w.out.p, &launches));
  TRY(download(c, weights_out, w.out.p, 8 * nc * n_groups));
  kw_reaching(weights_out, min_weight, n_groups, nc, w.reach);
  const size_t nr = w.reach.size();
  c->kw.stat[0] += n_groups; c->kw.stat[1] += n_groups - nr; c->kw.stat[2] += launches;
  if (nr == n_groups) return ks_verify_rows(c, k, nullptr, msgs, off, sigs, n_groups, dst, dst_len, valid_bitmap);
  std::memset(valid_bitmap, 0, nb);
  if (nr == 0) return 0;
  // the sub-call of the reaching groups (ctx-owned: the arrays outlive the asynchronous uploads)
  kw_repack(w.reach, sel, rb, msgs, off, sigs, w.sub);
  w.h_bits.assign((nr + 7) / 8, 0);
  TRY(ks_verify_rows(c, k, w.sub.rows.data(), w.sub.msgs.data(), w.sub.off.data(), w.sub.sigs.data(), nr, dst, dst_len, w.h_bits.data()));
  kw_scatter_bits(w.reach, w.h_bits.data(), valid_bitmap);
  return 0;
}

int blsbn254_keyset_weight_stats(blsbn254_ctx* c, uint64_t out[4]) { return COPY_STATS(c, kw.stat, 4, out); }

}  // extern "C"
