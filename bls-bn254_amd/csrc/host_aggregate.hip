// host_aggregate.hip -- the aggregate family: aggregate verify (per-key sums, pair by pair, sharded partial / finish, over prepared
// keys) and the Miller product over prepared keys; signature aggregation, threshold combine and Lagrange coefficients.  Host side of
// include/blsbn254.h; see host_common.h.
// What the calls that run Miller loops off the RAW line tables share is here, each written once: launch_miller_raw (THE size rule
// of that loop; host_aggregate_rlc.hip's rounds take it too), agg_keys_stage / agg_keys_prepare (the call's keys and -G2gen as
// tables beside the hashing), product_bytes / product_is_one over fp12_tree, and the verdict words (VW_*) the calls read back.
#include "host_common.h"

extern "C" {

// in-place product tree over `cnt` Fp12 values at a (stride sa); result pointer / stride returned
int fp12_tree(blsbn254_ctx* c, int32_t* a, size_t cnt, size_t sa, int32_t** res, size_t* rs) {
  HIPCHK(c, c->f_ws2.reserve(((cnt + 1) / 2) * 108 * 4 + 432));
  int32_t* b = (int32_t*)c->f_ws2.p;
  while (cnt > 1) {
    size_t mo = (cnt + 1) / 2;
    TRY(launch(c, c->stream, "fp12_mul_pairs", grid_lanes(mo), k_fp12_mul_pairs, (const int32_t*)a, cnt, sa, b, mo));
    std::swap(a, b); sa = mo; cnt = mo;
  }
  *res = a; *rs = sa;
  return 0;
}
// the product of the cnt values at f (stride cnt) as 384 bytes: the copy into `out` is enqueued, the caller waits for the stream
static int product_bytes(blsbn254_ctx* c, int32_t* f, size_t cnt, uint8_t out[384]) {
  int32_t* res; size_t rs;
  HIPCHK(c, c->out.reserve(384));
  TRY(fp12_tree(c, f, cnt, cnt, &res, &rs));
  TRY(launch(c, c->stream, "fp12_to_bytes", grid_lanes(1), k_fp12_to_bytes, (const int32_t*)res, (size_t)1, rs, (uint8_t*)c->out.p));
  HIPCHK(c, hipMemcpyAsync(out, c->out.p, 384, hipMemcpyDeviceToHost, c->stream));
  return 0;
}
// ... or ONE final exponentiation of it: 1 into *d_is_one where the result is one (enqueued)
static int product_is_one(blsbn254_ctx* c, int32_t* f, size_t cnt, int* d_is_one) {
  int32_t* res; size_t rs;
  TRY(fp12_tree(c, f, cnt, cnt, &res, &rs));
  return run_final_exp(c, res, 1, rs, 3, nullptr, nullptr, nullptr, nullptr, d_is_one);
}
// The verdict words of a call, in c->misc: the first key index out of range (check_key_indices folds it into word 0: the calls over
// a caller's indices), all keys valid (k_and_reduce), the signature's validity byte (k_g1_to_ws), the is-one word of product_is_one.
// verdict_arm: {NO_INDEX, 1, 1} in ONE upload from a static source; verdict_read: all of them, synchronised.
enum { VW_INDEX = 0, VW_KEYS = 1, VW_SIG = 2, VW_IS_ONE = 4, VW_WORDS = 5 };
static int verdict_arm(blsbn254_ctx* c, int** d) {
  static const int init[3] = {NO_INDEX, 1, 1};
  HIPCHK(c, c->misc.reserve(64));
  *d = (int*)c->misc.p;
  return upload(c, c->misc, init, sizeof init);
}
static int verdict_read(blsbn254_ctx* c, int h[VW_WORDS]) { return download(c, h, c->misc.p, 4 * VW_WORDS); }

// The table-only Miller loop over n pairs off the raw line tables, in the form launch_forms.h names
int launch_miller_raw(blsbn254_ctx* c, const int32_t* h, size_t h_stride, const uint32_t* kid, RawTables kt, size_t n, const uint8_t* st, unsigned forms,
                      size_t* left) {
  const bool two = raw_two_per_lane(c->forms, n, forms, c->chunk);
  *left = two ? (n + 1) / 2 : n;
  HIPCHK(c, c->f_ws.reserve(*left * 108 * 4)); HIPCHK(c, c->flags.reserve(n));
  int32_t* f = (int32_t*)c->f_ws.p; uint8_t* flags = (uint8_t*)c->flags.p;
  if (two) return launch(c, c->stream, "miller_hpk2p", grid_lanes(*left), k_miller_hpk2p, h, h_stride, kid, kt.raw, kt.ok, n, f, *left, flags, st);
  return for_chunks(c, n, [&](size_t lo, size_t m) -> int {
    const uint8_t* s = st ? st + lo : nullptr;
    switch (table_miller_form(c->forms, m, forms)) {
      case Form::WIDE: return launch(c, c->stream, "miller_wide_1p", grid_wide(m), k_miller_wide_1p, h + lo, h_stride, kid + lo, kt.raw, kt.ok, m, f + lo, n, flags + lo, s);
      case Form::TRI: return launch(c, c->stream, "miller_tri_1p", grid_tri(m), k_miller_tri_1p, h + lo, h_stride, kid + lo, kt.raw, kt.ok, m, f + lo, n, flags + lo, s);
      case Form::LANE: break;
    }
    return launch(c, c->stream, "miller_hpk1p", grid_lanes(m), k_miller_hpk1p, h + lo, h_stride, kid + lo, kt.raw, kt.ok, m, f + lo, n, flags + lo, s);
  });
}
int agg_keys_stage(blsbn254_ctx* c, const uint8_t* pks, size_t n, size_t* u) {
  HIPCHK(c, c->in_a.reserve(128 * (n + 1)));
  HIPCHK(c, hipMemcpyAsync(c->in_a.p, pks, 128 * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync((uint8_t*)c->in_a.p + 128 * n, NEG_G2_BYTES, 128, hipMemcpyHostToDevice, c->stream));   // "pair n": the key of the signatures' pairs
  return dedup_keys(c, (const uint8_t*)c->in_a.p, n, u);
}
// the `keys` keys of c->in_a that kd.keys names become raw line tables on the second stream, ev_join behind them
int raw_tables_fork(blsbn254_ctx* c, size_t keys) {
  HIPCHK(c, c->prep.ok.reserve(keys)); HIPCHK(c, c->prep.raw.reserve(keys * PREP_RAW_LIMBS * 4));
  HIPCHK(c, fork_stream2(c));
  TRY(launch_g2_prepare(c, c->stream2, (const uint8_t*)c->in_a.p, (const uint32_t*)c->kd.keys.p, keys, (int32_t*)c->prep.raw.p, (uint8_t*)c->prep.ok.p, nullptr));
  HIPCHK(c, hipEventRecord(c->ev_join, c->stream2));
  return 0;
}
int agg_keys_prepare(blsbn254_ctx* c, size_t n, size_t u) {
  c->kd.last_key = (uint32_t)n;                            // context-owned: nothing waits for this copy (dedup_keys has waited for all before it)
  HIPCHK(c, hipMemcpyAsync((uint32_t*)c->kd.keys.p + u, &c->kd.last_key, 4, hipMemcpyHostToDevice, c->stream));
  return raw_tables_fork(c, u + 1);
}
// prod_i ML(H(msg_i), pk_i) over the caller's n pairs, optionally times ML(extra_sig, -G2gen): the aggregate signature
// then simply joins the batch as pair n (one more lane half among the million) instead of a latency-bound one-lane launch.
// Two pairs per lane sharing one f^2 (k_miller_hpk2), then the pairwise product tree.
// staged = true: the caller (aggregate_verify_grouped, which found the keys distinct) has already put dst, messages, keys and
// the signature where this function stages them
static int aggregate_partial_impl(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, size_t n,
                                  const uint8_t* dst, size_t dst_len, const uint8_t* extra_sig, uint8_t ml_out[384], int* all_pks_ok, int* sig_ok,
                                  bool staged = false) {
  Stream2Guard s2_guard(c);
  *all_pks_ok = 1;
  if (sig_ok) *sig_ok = 1;
  const size_t np = n + (extra_sig ? 1 : 0);                 // pairs in the loop
  if (np == 0) { std::memset(ml_out, 0, 384); ml_out[31] = 1; return 0; }
  CHECK_LANES(c, np);
  ENTER(c);
  uint32_t dl = 0;
  if (n) {
    TRY(stage_dst(c, dst, dst_len, &dl));                    // (a no-op when the tag is already resident)
    if (!staged) TRY(stage_msgs(c, msgs, off, n));
  }
  size_t left = (np + 1) / 2;                                // Fp12 values the loop leaves: one per lane
  HIPCHK(c, c->in_a.reserve(128 * np)); HIPCHK(c, c->in_b.reserve(64)); HIPCHK(c, c->h_ws.reserve(np * 18 * 4)); HIPCHK(c, c->f_ws.reserve(left * 108 * 4));
  HIPCHK(c, c->q_ws.reserve(left * 72 * 4)); HIPCHK(c, c->flags.reserve(np)); HIPCHK(c, c->sub_ok.reserve(np)); HIPCHK(c, c->misc.reserve(64)); HIPCHK(c, c->out.reserve(384));
  if (n && !staged) HIPCHK(c, hipMemcpyAsync(c->in_a.p, pks, 128 * n, hipMemcpyHostToDevice, c->stream));
  int* d_ok;
  TRY(verdict_arm(c, &d_ok));
  if (extra_sig && !staged) {
    HIPCHK(c, hipMemcpyAsync(c->in_b.p, extra_sig, 64, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync((uint8_t*)c->in_a.p + 128 * n, NEG_G2_BYTES, 128, hipMemcpyHostToDevice, c->stream));
  }
  // few distinct keys among the np pairs (the pair (sig, -G2gen) included)?  then prepare each once, beside the hashing
  // (agg_keys_stage / agg_keys_prepare do not fit: -G2gen is one of the np keys here, not one more, and only where a signature came)
  bool prepared = false;
  if (c->auto_prepare && np >= 1024) {
    size_t u = 0;
    TRY(dedup_keys(c, (const uint8_t*)c->in_a.p, np, &u));
    if (u * 2 <= np && u <= PREP_MAX_KEYS) {
      HIPCHK(c, c->prep.table.reserve(64));
      TRY(raw_tables_fork(c, u));
      TRY(dedup_key_ids(c, np, u, false));   // no sorting here: no histogram
      prepared = true;
    }
  }
  // hash (and, on the exact path, key checks) over the caller's n pairs; their H points land in slots 0..n-1 of a stride-np workspace
  if (n) {
    TRY(launch_hash_to_g1(c, c->stream, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, n, dl, (int32_t*)c->h_ws.p,
               np, (uint8_t*)nullptr, 0));
    if (!prepared) TRY(launch(c, c->stream, "g2_check", grid_lanes(n), k_g2_check, (const uint8_t*)c->in_a.p, n, (uint8_t*)c->sub_ok.p, (uint8_t*)nullptr));
  }
  if (extra_sig) TRY(launch(c, c->stream, "g1_to_ws", grid_lanes(1), k_g1_to_ws, (const uint8_t*)c->in_b.p, (int32_t*)c->h_ws.p, n, np, (uint8_t*)(d_ok + VW_SIG)));
  if (prepared) {
    // few distinct keys: every key (and -G2gen, when the signature's pair is carried) was validated and turned into its line
    // table once, beside hash-to-G1; the pairs read their lines from those tables
    HIPCHK(c, join_stream2(c));
    TRY(launch_miller_raw(c, (const int32_t*)c->h_ws.p, np, (const uint32_t*)c->kd.kid.p, {(const int32_t*)c->prep.raw.p, (const uint8_t*)c->prep.ok.p}, np, nullptr,
                          MR_TWO, &left));
  } else {
    TRY(launch(c, c->stream, "miller_hpk2", grid_lanes(left), k_miller_hpk2, (const int32_t*)c->h_ws.p, (const uint8_t*)c->in_a.p, np, (int32_t*)c->q_ws.p,
               (int32_t*)c->f_ws.p, left, (uint8_t*)c->flags.p));
  }
  if (n) TRY(launch(c, c->stream, "and_reduce", grid_lanes(n), k_and_reduce, (const uint8_t*)c->flags.p, (const uint8_t*)(prepared ? c->flags.p : c->sub_ok.p), n, d_ok + VW_KEYS));
  TRY(product_bytes(c, (int32_t*)c->f_ws.p, left, ml_out));
  int h[VW_WORDS];
  TRY(verdict_read(c, h));
  *all_pks_ok = h[VW_KEYS];
  if (sig_ok) *sig_ok = (h[VW_SIG] & 0xff) == 1;
  return 0;
}
int blsbn254_aggregate_partial(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, size_t n,
                               const uint8_t* dst, size_t dst_len, uint8_t ml_out[384], int* all_pks_ok) {
  if (!c || !ml_out || !all_pks_ok || !off || (n && !pks) || (dst_len && !dst)) return BLSBN254_E_ARG;
  return aggregate_partial_impl(c, pks, msgs, off, n, dst, dst_len, nullptr, ml_out, all_pks_ok, nullptr);
}
// The first shard of a sharded aggregate verify may carry the aggregate signature's pair as well (then the finishing
// call passes agg_sig = NULL): *sig_ok = the signature decodes, is not the identity and is on the curve.
int blsbn254_aggregate_partial_with_sig(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, size_t n,
                                        const uint8_t* dst, size_t dst_len, const uint8_t agg_sig[64], uint8_t ml_out[384], int* all_pks_ok, int* sig_ok) {
  if (!c || !ml_out || !all_pks_ok || !sig_ok || !agg_sig || !off || (n && !pks) || (dst_len && !dst)) return BLSBN254_E_ARG;
  return aggregate_partial_impl(c, pks, msgs, off, n, dst, dst_len, agg_sig, ml_out, all_pks_ok, sig_ok);
}
int blsbn254_aggregate_finish(blsbn254_ctx* c, const uint8_t* partials, size_t k, const uint8_t agg_sig[64], int* valid) {
  if (!c || !valid || (k && !partials) || (!k && !agg_sig)) return BLSBN254_E_ARG;
  *valid = 0;
  ENTER(c);
  const bool with_sig = agg_sig != nullptr;                // NULL: a partial already carries ML(agg_sig, -G2gen)
  size_t m = k + (with_sig ? 1 : 0);                       // slot k holds ML(agg_sig, -G2gen)
  HIPCHK(c, c->in_a.reserve(384 * (k ? k : 1))); HIPCHK(c, c->in_b.reserve(64 + 128)); HIPCHK(c, c->f_ws.reserve(m * 108 * 4));
  HIPCHK(c, c->status.reserve(k + 8)); HIPCHK(c, c->misc.reserve(64)); HIPCHK(c, c->bitmap.reserve(16));
  int32_t* f = (int32_t*)c->f_ws.p;
  if (with_sig) {
    uint8_t last[64 + 128];
    std::memcpy(last, agg_sig, 64); std::memcpy(last + 64, NEG_G2_BYTES, 128);
    HIPCHK(c, hipMemcpyAsync(c->in_b.p, last, sizeof last, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));       // `last` is on the stack
  }
  if (k) {
    HIPCHK(c, hipMemcpyAsync(c->in_a.p, partials, 384 * k, hipMemcpyHostToDevice, c->stream));
    // partials arrive as bytes: decode into slots 0..k-1 of the stride-m array
    TRY(launch(c, c->stream, "fp12_from_bytes", grid_lanes(k), k_fp12_from_bytes, (const uint8_t*)c->in_a.p, k, f, m, (uint8_t*)c->status.p));
    int bad;
    TRY(first_bad(c, (const uint8_t*)c->status.p, k, 1, 1, &bad));
    if (bad >= 0) return BLSBN254_ERR_GT;
  }
  if (with_sig) {
    TRY(launch(c, c->stream, "miller_1", grid_lanes(1), k_miller_1, (const uint8_t*)c->in_b.p, (const uint8_t*)c->in_b.p + 64, (size_t)1, f + k, m, (uint8_t*)c->status.p));
    TRY(launch(c, c->stream, "g1_check", grid_lanes(1), k_g1_check, (const uint8_t*)c->in_b.p, (size_t)1, (uint8_t*)c->bitmap.p));
  }
  int* d_one = (int*)c->misc.p + VW_IS_ONE;
  TRY(product_is_one(c, f, m, d_one));
  int h_one = 0; uint8_t sig_st = 3, sig_on_curve = 1;
  HIPCHK(c, hipMemcpyAsync(&h_one, d_one, 4, hipMemcpyDeviceToHost, c->stream));
  if (with_sig) {
    HIPCHK(c, hipMemcpyAsync(&sig_st, c->status.p, 1, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&sig_on_curve, c->bitmap.p, 1, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  bool sig_ok = (sig_st & 7) == 3 && (sig_on_curve & 1);      // decodes, not the identity, on the curve
  *valid = (sig_ok && h_one == 1) ? 1 : 0;
  return 0;
}
// Aggregate verify over a batch that repeats public keys, by bilinearity in the first argument (exact, no randomness):
//   prod_i e(H_i, pk_(k_i)) = prod_k e( sum_{i: k_i = k} H_i , pk_k )
// so only one Miller loop per DISTINCT key (plus the signature's pair) runs, after n G1 additions: key de-duplication and
// key-sorted order as in verify_batch, the sums by levels of chunks of KEY_SUM_GROUP points (key_sums, k_g1_seg_sum), the u + 1 pairs on the
// table-only loop in the form that fits them (launch_miller_raw), product tree, ONE final exponentiation.  The boolean is aggregate_verify's; the Miller
// value is not the product of the n per-pair values (blsbn254_aggregate_partial keeps that bit-exact form for the sharded API).
// *took = false: keys do not repeat, nothing was done.
static int aggregate_verify_grouped(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, size_t n, const uint8_t agg_sig[64],
                                    const uint8_t* dst, size_t dst_len, int* valid, bool* took) {
  Stream2Guard s2_guard(c);
  *took = false;
  ENTER(c);
  uint32_t dl = 0;
  TRY(stage_dst(c, dst, dst_len, &dl));
  TRY(stage_msgs(c, msgs, off, n));
  HIPCHK(c, c->in_a.reserve(128 * (n + 1)));
  TRY(upload(c, c->in_b, agg_sig, 64));
  size_t u = 0;
  TRY(agg_keys_stage(c, pks, n, &u));
  // few pairs: from tables, one wave or a quad of lanes per pair, whatever the keys
  const bool small = small_for_prepared(c->forms, n + 1, false);      // n + 1: the signature's pair joins the launch; one final exponentiation in all
  if (!((u * 2 <= n || small) && u + 1 <= PREP_MAX_KEYS)) return 0;
  *took = true;
  const size_t np = u + 1;
  TRY(agg_keys_prepare(c, n, u));                                               // the u keys and -G2gen (key id u), beside the hashing
  // key ids, key-sorted order
  HIPCHK(c, c->h_ws.reserve(n * 27 * 4)); HIPCHK(c, c->f_ws.reserve((np + 1) / 2 * 108 * 4)); HIPCHK(c, c->flags.reserve(np)); HIPCHK(c, c->status.reserve(np + 8)); HIPCHK(c, c->misc.reserve(64));
  HIPCHK(c, c->rlc.b.reserve(np * 18 * 4)); HIPCHK(c, c->rlc.idx.reserve(4 * np));
  TRY(dedup_key_ids(c, n, u, true));
  TRY(key_sorted_order(c, (const uint32_t*)c->kd.kid.p, n, u));                 // cursor[k] is now the END of run k
  const uint32_t *hist = (const uint32_t*)c->kd.hist.p, *cursor = (const uint32_t*)c->kd.cursor.p, *perm = (const uint32_t*)c->kd.perm.p, *kid = (const uint32_t*)c->kd.kid.p;
  TRY(launch_hash_to_g1(c, c->stream, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, n, dl, (int32_t*)c->h_ws.p, n,
             (uint8_t*)nullptr, 3));
  // sums per key: the tuples in sorted order (columns perm[s] of h_ws) -> one sum per key (key_sums)
  const int32_t* pts = nullptr; size_t pts_stride = u;
  TRY(key_sums(c, (const int32_t*)c->h_ws.p, nullptr, n, perm, perm, kid, hist, cursor, n, u, &pts, nullptr));
  // the u + 1 pairs: (sum_k, pk_k) for k < u and (agg_sig, -G2gen) as pair u with key id u
  int32_t* h2 = (int32_t*)c->rlc.b.p; uint8_t* st = (uint8_t*)c->status.p; uint32_t* kid2 = (uint32_t*)c->rlc.idx.p;   // (RlcWs: the buffers of whichever call runs)
  int* d_ok;
  TRY(verdict_arm(c, &d_ok));
  TRY(launch(c, c->stream, "g1p_to_h", grid_lanes(u), k_g1p_to_h_affine, pts, pts_stride, u, h2, np, st));
  HIPCHK(c, hipMemsetAsync(st + u, 1, 1, c->stream));
  TRY(launch(c, c->stream, "g1_to_ws", grid_lanes(1), k_g1_to_ws, (const uint8_t*)c->in_b.p, h2, u, np, (uint8_t*)(d_ok + VW_SIG)));
  TRY(launch(c, c->stream, "iota", grid_lanes(np), k_iota_u32, kid2, (uint32_t)np));
  HIPCHK(c, join_stream2(c));
  size_t left;
  TRY(launch_miller_raw(c, h2, np, kid2, {(const int32_t*)c->prep.raw.p, (const uint8_t*)c->prep.ok.p}, np, st, MR_ALL, &left));
  TRY(launch(c, c->stream, "and_reduce", grid_lanes(u), k_and_reduce, (const uint8_t*)c->flags.p, (const uint8_t*)c->flags.p, u, d_ok + VW_KEYS));
  TRY(product_is_one(c, (int32_t*)c->f_ws.p, left, d_ok + VW_IS_ONE));
  int h[VW_WORDS];
  TRY(verdict_read(c, h));
  *valid = (h[VW_KEYS] == 1 && (h[VW_SIG] & 0xff) == 1 && h[VW_IS_ONE] == 1) ? 1 : 0;
  ++c->agg_stat[0];
  return 0;
}
int blsbn254_aggregate_verify(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, size_t n,
                              const uint8_t agg_sig[64], const uint8_t* dst, size_t dst_len, int* valid) {
  if (!c || !valid || !agg_sig || !off || (n && !pks) || (dst_len && !dst)) return BLSBN254_E_ARG;
  *valid = 0;
  if (n == 0) return 0;
  if (n + 1 > MAX_LANES) { c->last_error = "more than 2^23 - 1 pairs in one aggregate_verify call"; return BLSBN254_E_ARG; }
  uint8_t ml[384]; int ok = 0, sig_ok = 0, v = 0;
  bool staged = false;
  if (c->auto_prepare && (n >= 1024 || grouped_whatever_keys(c->forms, n + 1))) {   // repeated keys (or few pairs): one pair per distinct key
    bool took = false;
    TRY(aggregate_verify_grouped(c, pks, msgs, off, n, agg_sig, dst, dst_len, valid, &took));
    if (took) return 0;
    staged = true;
  }
  ++c->agg_stat[1];
  TRY(aggregate_partial_impl(c, pks, msgs, off, n, dst, dst_len, agg_sig, ml, &ok, &sig_ok, staged));
  TRY(blsbn254_aggregate_finish(c, ml, 1, nullptr, &v));
  *valid = (ok == 1 && sig_ok == 1 && v == 1) ? 1 : 0;
  return 0;
}
// multi_miller_loop(&[(&G1Affine, &G2Prepared)]) (pairings.rs:808-857) over prepared keys named by index: the Fp12 product of
// the n Miller values, one wave per pair or two pairs per lane sharing f^2, every line read from the keys' tables.  A pair whose G1 member is
// the identity contributes 1 (the reference skips such terms); every referenced key must be valid (else InvalidG2Bytes).
int blsbn254_multi_miller_loop_prepared(blsbn254_ctx* c, const blsbn254_g2prepared* keys, const uint32_t* key_idx, const uint8_t* g1, size_t n,
                                        uint8_t ml_out[384]) {
  if (!c || !keys || keys->ctx != c || !ml_out || (n && (!key_idx || !g1))) return BLSBN254_E_ARG;
  if (n == 0) { std::memset(ml_out, 0, 384); ml_out[31] = 1; return 0; }
  CHECK_LANES(c, n);
  ENTER(c);
  HIPCHK(c, c->h_ws.reserve(n * 18 * 4)); HIPCHK(c, c->status.reserve(n)); HIPCHK(c, c->kd.hist.reserve(4 * (keys->u + 1)));
  TRY(upload(c, c->in_a, g1, 64 * n));
  TRY(upload(c, c->kd.kid, key_idx, 4 * n));
  TRY(check_key_indices(c, (const uint32_t*)c->kd.kid.p, n, keys->u, (uint32_t*)c->kd.hist.p, "pair", false));
  int bad;
  TRY(launch(c, c->stream, "g1_to_ws", grid_lanes(n), k_g1_to_ws_batch, (const uint8_t*)c->in_a.p, n, (int32_t*)c->h_ws.p, (uint8_t*)c->status.p));
  TRY(first_bad(c, (const uint8_t*)c->status.p, n, 1, 1, &bad));
  if (bad >= 0) return BLSBN254_ERR_G1;
  size_t left;                                               // few pairs: one wave per pair, product of n values instead of n / 2
  TRY(launch_miller_raw(c, (const int32_t*)c->h_ws.p, n, (const uint32_t*)c->kd.kid.p, {(const int32_t*)keys->raw.p, (const uint8_t*)keys->ok.p}, n,
                        (const uint8_t*)c->status.p, MR_WIDE | MR_TWO, &left));
  TRY(first_bad(c, (const uint8_t*)c->flags.p, n, 1, 1, &bad));
  if (bad >= 0) return BLSBN254_ERR_G2;
  TRY(product_bytes(c, (int32_t*)c->f_ws.p, left, ml_out));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
// CoreAggregateVerify with the public keys given as prepared keys by index: prod_i e(H(msg_i), pk_[key_idx_i]) * e(agg_sig, -G2gen) == 1.
// The signature's pair uses the table's own -G2gen entry; two pairs per lane, every line from the tables, ONE final exponentiation.
int blsbn254_aggregate_verify_prepared(blsbn254_ctx* c, const blsbn254_g2prepared* keys, const uint32_t* key_idx, const uint8_t* msgs, const uint64_t* off,
                                       size_t n, const uint8_t agg_sig[64], const uint8_t* dst, size_t dst_len, int* valid) {
  if (!c || !keys || keys->ctx != c || !valid || !agg_sig || !off || (n && !key_idx) || (dst_len && !dst)) return BLSBN254_E_ARG;
  *valid = 0;
  if (n == 0) return 0;
  const size_t np = n + 1;
  CHECK_LANES(c, np);
  ENTER(c);
  uint32_t dl;
  TRY(stage_dst(c, dst, dst_len, &dl));
  TRY(stage_msgs(c, msgs, off, n));
  HIPCHK(c, c->in_b.reserve(64)); HIPCHK(c, c->kd.kid.reserve(4 * np)); HIPCHK(c, c->h_ws.reserve(np * 18 * 4)); HIPCHK(c, c->kd.hist.reserve(4 * (keys->u + 2)));
  const uint32_t sig_key = (uint32_t)keys->u;
  HIPCHK(c, hipMemcpyAsync(c->kd.kid.p, key_idx, 4 * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync((uint32_t*)c->kd.kid.p + n, &sig_key, 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->in_b.p, agg_sig, 64, hipMemcpyHostToDevice, c->stream));
  int* d_ok;
  TRY(verdict_arm(c, &d_ok));                           // the armed index shares its upload with the two validity words
  TRY(check_key_indices(c, (const uint32_t*)c->kd.kid.p, n, keys->u, (uint32_t*)c->kd.hist.p, "pair", true));   // its read-back also waits for the copy of sig_key (on the stack)
  TRY(launch_hash_to_g1(c, c->stream, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, n, dl, (int32_t*)c->h_ws.p, np,
             (uint8_t*)nullptr, 0));
  TRY(launch(c, c->stream, "g1_to_ws", grid_lanes(1), k_g1_to_ws, (const uint8_t*)c->in_b.p, (int32_t*)c->h_ws.p, n, np, (uint8_t*)(d_ok + VW_SIG)));
  size_t left;
  TRY(launch_miller_raw(c, (const int32_t*)c->h_ws.p, np, (const uint32_t*)c->kd.kid.p, {(const int32_t*)keys->raw.p, (const uint8_t*)keys->ok.p}, np, nullptr,
                        MR_TWO, &left));
  TRY(launch(c, c->stream, "and_reduce", grid_lanes(n), k_and_reduce, (const uint8_t*)c->flags.p, (const uint8_t*)c->flags.p, n, d_ok + VW_KEYS));
  TRY(product_is_one(c, (int32_t*)c->f_ws.p, left, d_ok + VW_IS_ONE));
  int h[VW_WORDS];
  TRY(verdict_read(c, h));
  *valid = (h[VW_KEYS] == 1 && (h[VW_SIG] & 0xff) == 1 && h[VW_IS_ONE] == 1) ? 1 : 0;
  return 0;
}
// n G1 points (limb-major projective, stride n) in c->h_ws -> their sum as 64 bytes
int g1_sum_to_bytes(blsbn254_ctx* c, size_t n, uint8_t out[64]) {
  HIPCHK(c, c->f_ws2.reserve(((n + 1) / 2) * 27 * 4)); HIPCHK(c, c->out.reserve(64));
  int32_t* a = (int32_t*)c->h_ws.p; int32_t* b = (int32_t*)c->f_ws2.p;
  size_t sa = n, cnt = n;
  while (cnt > 1) {
    size_t mo = (cnt + 1) / 2;
    TRY(launch(c, c->stream, "g1_add_pairs", grid_lanes(mo), k_g1_add_pairs, (const int32_t*)a, cnt, sa, b, mo));
    std::swap(a, b); sa = mo; cnt = mo;
  }
  TRY(launch(c, c->stream, "g1_to_bytes", grid_lanes(1), k_g1_to_bytes, (const int32_t*)a, sa, (uint8_t*)c->out.p));
  return download(c, out, c->out.p, 64);
}
int blsbn254_aggregate_sigs(blsbn254_ctx* c, const uint8_t* sigs, size_t n, uint8_t out[64]) {
  if (!c || !out || (n && !sigs)) return BLSBN254_E_ARG;
  if (n == 0) { std::memset(out, 0, 64); out[63] = 1; return 0; }            // empty sum = identity (0, 1)
  ENTER(c);
  HIPCHK(c, c->h_ws.reserve(n * 27 * 4)); HIPCHK(c, c->status.reserve(n));
  TRY(upload(c, c->in_a, sigs, 64 * n));
  TRY(launch(c, c->stream, "g1_load", grid_lanes(n), k_g1_load, (const uint8_t*)c->in_a.p, n, (int32_t*)c->h_ws.p, (uint8_t*)c->status.p));
  int bad; int rc = first_bad(c, (const uint8_t*)c->status.p, n, 1, 1, &bad);
  if (rc) return rc;
  if (bad >= 0) return BLSBN254_ERR_G1;
  return g1_sum_to_bytes(c, n, out);
}
// The first half of threshold_combine and lagrange_at_zero: t ids (32 bytes each, the caller's) -> their Lagrange coefficients at
// zero in c->scalars (t x 32 bytes big-endian) and as GLV halves in c->th.glv, over t x S lanes (S ~ sqrt(t) slices: critical
// path 2 (t / S + S) products).  Left for the caller: the ids' decode status in c->status[0 .. t) (room for t more bytes behind
// them), their duplicate marks in c->flags, and two armed "first bad index" words at c->misc.
static int lagrange_enqueue(blsbn254_ctx* c, const uint8_t* ids, size_t t) {
  size_t S = 1;
  while (S < 64 && S * S < t) ++S;
  const size_t J = (t + S - 1) / S;
  HIPCHK(c, c->scalars.reserve(32 * t)); HIPCHK(c, c->status.reserve(2 * t)); HIPCHK(c, c->flags.reserve(t)); HIPCHK(c, c->misc.reserve(64));
  HIPCHK(c, c->th.x.reserve(9 * t * 4)); HIPCHK(c, c->th.num.reserve(9 * t * S * 4)); HIPCHK(c, c->th.den.reserve(9 * t * S * 4)); HIPCHK(c, c->th.glv.reserve(9 * t * 4));
  uint8_t* dup = (uint8_t*)c->flags.p;
  TRY(upload(c, c->in_b, ids, 32 * t));
  TRY(min_index_arm(c, (int*)c->misc.p, 2));
  HIPCHK(c, hipMemsetAsync(dup, 0, t, c->stream));
  TRY(launch(c, c->stream, "fr_decode", grid_lanes(t), k_fr_decode, (const uint8_t*)c->in_b.p, t, (int32_t*)c->th.x.p, (uint8_t*)c->status.p));
  TRY(launch(c, c->stream, "lagrange_partial", Shape{dim3(nblocks(t), (unsigned)S), dim3(256)}, k_lagrange_partial, (const int32_t*)c->th.x.p, t, J,
             (int32_t*)c->th.num.p, (int32_t*)c->th.den.p, dup));
  return launch(c, c->stream, "lagrange_finish", grid_lanes(t), k_lagrange_finish, (const int32_t*)c->th.num.p, (const int32_t*)c->th.den.p, t, S, (uint8_t*)c->scalars.p,
                (uint32_t*)c->th.glv.p);
}
// ... and the ids' checks, folded into misc[0]: decoded, non-zero (status 1) and pairwise distinct (dup 0)
static int lagrange_ids_reduce(blsbn254_ctx* c, size_t t) {
  TRY(launch(c, c->stream, "status_reduce", grid_lanes(t), k_status_reduce, (const uint8_t*)c->status.p, t, (uint8_t)1, (uint8_t)1, (int*)c->misc.p));
  return launch(c, c->stream, "status_reduce", grid_lanes(t), k_status_reduce, (const uint8_t*)c->flags.p, t, (uint8_t)1, (uint8_t)0, (int*)c->misc.p);
}
// Threshold combine (k_threshold.hip): Lagrange coefficients over t x sqrt(t) lanes, GLV-split 4-bit-window MSM over
// 2t x 32 lanes with in-workgroup sums, one short finishing kernel.  One host synchronisation at the end.
// (the body of blsbn254_threshold_combine for one group of 1 <= t <= MAX_LANES shares, after ENTER; the batched form sends its
// large groups through it, host_threshold_batch.hip)
int threshold_combine_one(blsbn254_ctx* c, const uint8_t* ids, const uint8_t* partial_sigs, size_t t, uint8_t out_sig[64]) {
  size_t n_chunks = (2 * t + 255) / 256;
  HIPCHK(c, c->out.reserve(64)); HIPCHK(c, c->th.part.reserve(27 * 32 * n_chunks * 4)); HIPCHK(c, c->th.part2.reserve(27 * 32 * ((n_chunks + 1) / 2) * 4));
  TRY(upload(c, c->in_a, partial_sigs, 64 * t));
  TRY(lagrange_enqueue(c, ids, t));
  uint8_t* st_pts = (uint8_t*)c->status.p + t;
  int* d_bad = (int*)c->misc.p;
  TRY(launch(c, c->stream, "msm_window", Shape{dim3((unsigned)n_chunks, 32), dim3(256)}, k_msm_window, (const uint8_t*)c->in_a.p, (const uint32_t*)c->th.glv.p, t,
             (int32_t*)c->th.part.p, st_pts));
  int32_t* pa = (int32_t*)c->th.part.p; int32_t* pb = (int32_t*)c->th.part2.p;
  while (n_chunks > 16) {                                  // large t only: fold the chunk axis pairwise
    const size_t no = (n_chunks + 1) / 2;
    TRY(launch(c, c->stream, "msm_fold", grid_lanes(no * 32), k_msm_fold, (const int32_t*)pa, n_chunks, pb));
    std::swap(pa, pb); n_chunks = no;
  }
  TRY(launch(c, c->stream, "msm_finish", Shape{dim3(1), dim3(64)}, k_msm_finish, (const int32_t*)pa, n_chunks, (uint8_t*)c->out.p));
  TRY(lagrange_ids_reduce(c, t));
  TRY(launch(c, c->stream, "status_reduce", grid_lanes(t), k_status_reduce, (const uint8_t*)st_pts, t, (uint8_t)1, (uint8_t)1, d_bad + 1));   // points: decoded
  int bad[2];
  HIPCHK(c, hipMemcpyAsync(bad, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
  TRY(download(c, out_sig, c->out.p, 64));
  if (bad[0] != NO_INDEX) return BLSBN254_ERR_SCALAR;
  if (bad[1] != NO_INDEX) return BLSBN254_ERR_G1;
  return 0;
}
int blsbn254_threshold_combine(blsbn254_ctx* c, const uint8_t* ids, const uint8_t* partial_sigs, size_t t, uint8_t out_sig[64]) {
  if (!c || !out_sig || (t && (!ids || !partial_sigs))) return BLSBN254_E_ARG;
  if (t == 0) { std::memset(out_sig, 0, 64); out_sig[63] = 1; return 0; }
  CHECK_LANES(c, t);
  ENTER(c);
  return threshold_combine_one(c, ids, partial_sigs, t, out_sig);
}
// The Lagrange coefficients at zero alone (t x 32 bytes big-endian), for callers that combine elsewhere and for tests.
// (lagrange_one: the body for 1 <= t <= MAX_LANES ids, after ENTER)
int lagrange_one(blsbn254_ctx* c, const uint8_t* ids, size_t t, uint8_t* out) {
  TRY(lagrange_enqueue(c, ids, t));
  TRY(lagrange_ids_reduce(c, t));
  int bad;
  HIPCHK(c, hipMemcpyAsync(&bad, c->misc.p, 4, hipMemcpyDeviceToHost, c->stream));
  TRY(download(c, out, c->scalars.p, 32 * t));
  return bad != NO_INDEX ? BLSBN254_ERR_SCALAR : 0;
}
int blsbn254_lagrange_at_zero(blsbn254_ctx* c, const uint8_t* ids, size_t t, uint8_t* out) {
  if (!c || (t && (!ids || !out))) return BLSBN254_E_ARG;
  if (t == 0) return 0;
  CHECK_LANES(c, t);
  ENTER(c);
  return lagrange_one(c, ids, t, out);
}


}  // extern "C"
