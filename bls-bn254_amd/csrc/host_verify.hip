// host_verify.hip -- batched BLS verify: key de-duplication, per-key line tables (G2Prepared), the table-only and the exact
// per-tuple pipelines, and the explicit G2Prepared API.  Host side of include/blsbn254.h; see host_common.h.
#include "host_common.h"

extern "C" {

// ---------------- verify
// G2Prepared::from for u keys (decode, on-curve, psi subgroup test, 88 line triples) on stream s, four lanes per key or one
int launch_g2_prepare(blsbn254_ctx* c, hipStream_t s, const uint8_t* pks, const uint32_t* keys, size_t u, int32_t* raw, uint8_t* ok, const uint32_t* d_u) {
  if (prepare_on_quads(c->forms, u))
    return launch(c, s, "g2_prepare", grid_lanes(2 * 256 * (size_t)nblocks(4 * u)), k_g2_prepare_quad, pks, keys, (uint32_t)u, raw, ok, d_u);
  return launch(c, s, "g2_prepare", grid_lanes(2 * 256 * (size_t)nblocks(u)), k_g2_prepare, pks, keys, (uint32_t)u, raw, ok, d_u);
}
// G2Prepared::from for at most u of the tuples `keys` names (u a capacity when d_u gives the count on the device), dense into
// prep.raw / prep.table / prep.ok, on the second stream
static int prepare_dense(blsbn254_ctx* c, const uint8_t* d_pks, const uint32_t* keys, size_t u, const uint32_t* d_u) {
  TRY(launch_g2_prepare(c, c->stream2, d_pks, keys, u, (int32_t*)c->prep.raw.p, (uint8_t*)c->prep.ok.p, d_u));
  return launch(c, c->stream2, "g2_expand", grid_lanes(u * (size_t)BN_NEG_G2_LINES), k_g2_expand, (const int32_t*)c->prep.raw.p, (uint32_t)u, (int32_t*)c->prep.table.p, d_u,
                (uint8_t*)c->prep.ok.p);
}
// ---- the store of prepared keys (key_cache.h, k_keycache.hip).  In real use a validator set's keys stay the same from batch to
// batch: a key whose 128 bytes an earlier call on this context prepared keeps its table in the store, and only the keys that
// are new to the context are prepared.  57 024 B of table + 128 B of encoding + 1 B per key (and 8 B of slot table); the default
// of 4096 keys is 234 MB of the 288 GB, allocated by the first call that uses it.
// The store with room for at least `need` keys: max(kc.max, need), so that an empty store takes the call's keys whatever kc.max
// is.  Growing it is a reallocation (DevBuf::reserve waits for the device) that empties it; the running totals stay.
static int kc_reserve(blsbn254_ctx* c, size_t need) {
  KeyStore& s = c->kc;
  if (!s.state.p) {
    HIPCHK(c, s.state.reserve(64));          // KC_STATE_WORDS words, then (at byte 32) KC_STAT_WORDS 64-bit totals
    HIPCHK(c, hipMemsetAsync(s.state.p, 0, 64, c->stream));
  }
  const size_t want = std::max(s.max, need);
  if (want <= s.cap) return 0;
  size_t m = 1;
  while (m < 2 * want) m <<= 1;
  s.cap = 0;
  HIPCHK(c, s.table.reserve(want * PREP_KEY_LIMBS * 4)); HIPCHK(c, s.keys.reserve(128 * want)); HIPCHK(c, s.valid.reserve(want));
  HIPCHK(c, s.slots.reserve(4 * m));
  HIPCHK(c, hipMemsetAsync(s.slots.p, 0xff, 4 * m, c->stream));
  HIPCHK(c, hipMemsetAsync(s.state.p, 0, 4 * KC_STATE_WORDS, c->stream));
  s.cap = want; s.mask = (uint32_t)(m - 1);
  return 0;
}
// The store's branch of prepare_keys, on the second stream: look the distinct keys up, prepare the misses as prepare_dense
// prepares all keys (bounded by the device-side miss count: with every key resident these launches leave at once) and copy
// their tables into the store.  Afterwards kc.slot_of[j] is key j's place in kc.table / kc.valid.  No host decision, no read-back.
static int prepare_into_store(blsbn254_ctx* c, const uint8_t* d_pks, size_t cap) {
  KeyStore& s = c->kc;
  uint32_t* st = (uint32_t*)s.state.p;
  unsigned long long* stats = (unsigned long long*)((uint8_t*)s.state.p + 32);
  const uint32_t key_words = (uint32_t)(PREP_KEY_LIMBS / 4);
  TRY(launch(c, c->stream2, "kd_cache_begin", Shape{dim3(1), dim3(1)}, k_kd_cache_begin, (const uint32_t*)c->kd.cnt.p, (uint32_t)cap, (uint32_t)s.max, (uint32_t)s.cap, st, stats));
  TRY(launch(c, c->stream2, "kd_cache_clear", grid_lanes((size_t)s.mask + 1), k_kd_cache_clear, (const uint32_t*)st, (uint32_t*)s.slots.p, s.mask + 1));
  TRY(launch(c, c->stream2, "kd_cache_lookup", grid_lanes(cap), k_kd_cache_lookup, d_pks, (const uint32_t*)c->kd.keys.p, st, (uint32_t*)s.slots.p, s.mask, c->kd.seed,
             (uint8_t*)s.keys.p, (uint32_t*)s.slot_of.p, (uint32_t*)s.miss_rep.p, (uint32_t*)s.miss_slot.p));
  TRY(prepare_dense(c, d_pks, (const uint32_t*)s.miss_rep.p, cap, st + KC_MISS));
  const size_t copy_blocks = std::min<size_t>(nblocks(cap * (size_t)key_words), 2048);
  return launch(c, c->stream2, "kd_cache_scatter", Shape{dim3((unsigned)copy_blocks), dim3(256)}, k_kd_cache_scatter, (const int4*)c->prep.table.p, (const uint8_t*)c->prep.ok.p,
                (const uint32_t*)s.miss_slot.p, key_words, st, stats, (int4*)s.table.p, (uint8_t*)s.valid.p);
}
// The prepared keys of the batch behind dedup_enqueue (kd.keys[j] = the representative tuple of the batch's distinct key j, kd.cnt
// of them on the device): see KeyTables in host_common.h.  THE place that chooses between the store and tables of this call:
// it reserves what the branch needs, forks, and records ev_join behind the branch's launches.  d_u bounds the work without a
// store, the miss count with one (a count beyond the capacity: the first `cap` keys are prepared or looked up, and
// verify_chunk_async's caller discards the run as before).
int prepare_keys(blsbn254_ctx* c, const uint8_t* d_pks, size_t cap, const uint32_t* d_u, KeyTables* kt) {
  KeyStore& s = c->kc;
  const bool store = s.max != 0;
  if (store) {
    TRY(kc_reserve(c, cap));
    HIPCHK(c, s.slot_of.reserve(4 * cap)); HIPCHK(c, s.miss_rep.reserve(4 * cap)); HIPCHK(c, s.miss_slot.reserve(4 * cap));
  }
  HIPCHK(c, c->prep.raw.reserve(cap * PREP_RAW_LIMBS * 4)); HIPCHK(c, c->prep.table.reserve(cap * PREP_KEY_LIMBS * 4)); HIPCHK(c, c->prep.ok.reserve(cap));
  HIPCHK(c, fork_stream2(c));
  TRY(store ? prepare_into_store(c, d_pks, cap) : prepare_dense(c, d_pks, (const uint32_t*)c->kd.keys.p, cap, d_u));
  HIPCHK(c, hipEventRecord(c->ev_join, c->stream2));
  *kt = store ? KeyTables{(const int32_t*)s.table.p, (const uint8_t*)s.valid.p, (const uint32_t*)s.slot_of.p}
              : KeyTables{(const int32_t*)c->prep.table.p, (const uint8_t*)c->prep.ok.p, nullptr};
  return 0;
}
// *out = the ids the Miller loops take for n elements given by batch key id: the ids themselves, or with a store its indices,
// mapped into buf on the main stream (after join_stream2)
int miller_ids(blsbn254_ctx* c, const KeyTables& kt, const uint32_t* ids, size_t n, DevBuf& buf, const uint32_t** out) {
  *out = ids;
  if (!kt.slot_of) return 0;
  HIPCHK(c, buf.reserve(4 * n));
  *out = (const uint32_t*)buf.p;
  return launch(c, c->stream, "kd_cache_map", grid_lanes(n), k_kd_cache_map, ids, (uint32_t)n, kt.slot_of, (uint32_t*)buf.p);
}
// *out = the u keys' validity bytes in batch key order: the tables' own, or gathered from the store's (after join_stream2)
int keys_valid(blsbn254_ctx* c, const KeyTables& kt, size_t u, const uint8_t** out) {
  *out = kt.ok;
  if (!kt.slot_of) return 0;
  HIPCHK(c, c->kc.batch_ok.reserve(u));
  *out = (const uint8_t*)c->kc.batch_ok.p;
  return launch(c, c->stream, "kd_cache_ok", grid_lanes(u), k_kd_cache_ok, kt.slot_of, (uint32_t)u, kt.ok, (uint8_t*)c->kc.batch_ok.p);
}
// Behind dedup_enqueue, on the main stream: every tuple's key id (kd.kid; ids beyond u clamped) and, hist: how many tuples each
// key has (kd.hist).  Then, from that histogram: the key-sorted order of the n tuples d_kid (kd.perm; kd.cursor[k] ends as the END
// of run k).  Two steps: verify_prepared_dev enqueues hash-to-G1 (and checks the explicit API's indices) between them.
int dedup_key_ids(blsbn254_ctx* c, size_t n, size_t u, bool hist) {
  if (hist) HIPCHK(c, hipMemsetAsync(c->kd.hist.p, 0, 4 * u, c->stream));
  return launch(c, c->stream, "kd_propagate", grid_lanes(n), k_kd_propagate, (const uint32_t*)c->kd.rep.p, (uint32_t)n, (uint32_t)u, (uint32_t*)c->kd.kid.p,
                hist ? (uint32_t*)c->kd.hist.p : nullptr);
}
int key_sorted_order(blsbn254_ctx* c, const uint32_t* d_kid, size_t n, size_t u) {
  HIPCHK(c, c->kd.cursor.reserve(4 * (u + 1))); HIPCHK(c, c->kd.perm.reserve(4 * n));
  TRY(launch(c, c->stream, "kd_scan", Shape{dim3(1), dim3(1024)}, k_scan_excl, (const uint32_t*)c->kd.hist.p, (uint32_t)u, (uint32_t*)c->kd.cursor.p));
  return launch(c, c->stream, "kd_scatter", grid_lanes(n), k_kd_scatter, d_kid, (uint32_t)n, (uint32_t)u, (uint32_t*)c->kd.cursor.p, (uint32_t*)c->kd.perm.p);
}
// Are all n key indices at d_kid below u?  k_kd_hist counts the keys into hist (zeroed here) and folds the first index out of
// range into misc[0]; read back (one 4-byte copy and a stream synchronisation).  armed: the caller has already put NO_INDEX there,
// in one upload with words of its own behind it.  `what` names the element in the error text ("tuple" / "pair").
int check_key_indices(blsbn254_ctx* c, const uint32_t* d_kid, size_t n, size_t u, uint32_t* hist, const char* what, bool armed) {
  if (!armed) { HIPCHK(c, c->misc.reserve(64)); TRY(min_index_arm(c, (int*)c->misc.p, 1)); }
  int* d_bad = (int*)c->misc.p;
  HIPCHK(c, hipMemsetAsync(hist, 0, 4 * u, c->stream));
  TRY(launch(c, c->stream, "kd_hist", grid_lanes(n), k_kd_hist, d_kid, (uint32_t)n, (uint32_t)u, hist, d_bad));
  int bad;
  TRY(min_index_read(c, d_bad, &bad));
  if (bad >= 0) { c->last_error = std::string("key index out of range at ") + what + " " + std::to_string(bad); return BLSBN254_E_ARG; }
  return 0;
}
// The table-only Miller loop over n tuples (f_ws, flags) in the form that fits n; the three forms give the same values.
int launch_miller_prepared(blsbn254_ctx* c, const uint32_t* perm, const uint32_t* kid, const uint8_t* sigs, const int32_t* h_ws, size_t h_stride, const KeyTables& kt, size_t n) {
  int32_t* f = (int32_t*)c->f_ws.p; uint8_t* flags = (uint8_t*)c->flags.p;
  switch (table_miller_form(c->forms, n)) {
    case Form::WIDE: return launch(c, c->stream, "miller_wide_prepared", grid_wide(n), k_miller_wide_prepared, perm, kid, sigs, h_ws, h_stride, kt.table, kt.ok, n, f, flags);
    case Form::TRI: return launch(c, c->stream, "miller_tri_prepared", grid_tri(n), k_miller_tri_prepared, perm, kid, sigs, h_ws, h_stride, kt.table, kt.ok, n, f, flags);
    case Form::LANE: break;
  }
  return launch(c, c->stream, "miller_prepared", grid_lanes(n), k_miller_prepared, perm, kid, sigs, h_ws, h_stride, kt.table, kt.ok, n, f, flags);
}
// Verify n tuples whose keys are given by index into prepared tables (d_kid[i] < u), everything device-resident.
// deduped: the ids are dedup_key_ids' -- their histogram is filled, and the tables' preparation is on stream2 (prepare_keys: ev_join).
// Else they are a caller's (checked here) and the tables are final.  The key ids give the key-sorted order whatever the
// tables; the Miller loop takes what miller_ids makes of them.
int verify_prepared_dev(blsbn254_ctx* c, const KeyTables& kt, size_t u, const uint32_t* d_kid, bool deduped, const uint8_t* d_msgs, const uint64_t* d_off,
                        const uint8_t* d_sigs, size_t n, uint32_t dl, uint8_t* d_bitmap) {
  HIPCHK(c, c->h_ws.reserve(n * 27 * 4)); HIPCHK(c, c->f_ws.reserve(n * 108 * 4)); HIPCHK(c, c->flags.reserve(n));
  HIPCHK(c, c->kd.hist.reserve(4 * (u + 1))); HIPCHK(c, c->prep.isone.reserve(n)); HIPCHK(c, c->prep.valid.reserve(n));
  TRY(launch_hash_to_g1(c, c->stream, d_msgs, d_off, n, dl, (int32_t*)c->h_ws.p, n, (uint8_t*)nullptr,
             3));   // homogeneous H: no inversion
  if (!deduped) TRY(check_key_indices(c, d_kid, n, u, (uint32_t*)c->kd.hist.p, "tuple", false));
  TRY(key_sorted_order(c, d_kid, n, u));
  if (deduped) HIPCHK(c, join_stream2(c));
  const uint32_t *perm = (const uint32_t*)c->kd.perm.p, *ids;
  TRY(miller_ids(c, kt, d_kid, n, c->kc.tslot, &ids));
  TRY(launch_miller_prepared(c, perm, ids, d_sigs, (const int32_t*)c->h_ws.p, n, kt, n));
  TRY(run_final_exp(c, (int32_t*)c->f_ws.p, n, n, 4, nullptr, nullptr, nullptr, (uint8_t*)c->prep.isone.p, nullptr));
  TRY(launch(c, c->stream, "prep_unsort", grid_lanes(n), k_prep_unsort, (const uint8_t*)c->prep.isone.p, (const uint8_t*)c->flags.p, perm, (uint32_t)n,
             (uint8_t*)c->prep.valid.p));
  return launch(c, c->stream, "pack_bitmap", grid_lanes(n), k_pack_bitmap, (const uint8_t*)c->prep.valid.p, n, d_bitmap);
}
// De-duplicate the public keys of a chunk: kd.rep / kd.kid / kd.keys and the count (kd.cnt) are filled on the device.
static int dedup_enqueue(blsbn254_ctx* c, const uint8_t* d_pks, size_t n) {
  size_t m = 1;
  while (m < 2 * n) m <<= 1;
  // n + 1 entries: aggregate_verify_grouped appends the key of the signature's pair (-G2gen) as entry u, and u can be n
  HIPCHK(c, c->kd.slots.reserve(4 * m)); HIPCHK(c, c->kd.rep.reserve(4 * (n + 1))); HIPCHK(c, c->kd.kid.reserve(4 * (n + 1))); HIPCHK(c, c->kd.keys.reserve(4 * (n + 1)));
  HIPCHK(c, c->kd.hist.reserve(4 * (n + 2))); HIPCHK(c, c->kd.cnt.reserve(64));
  HIPCHK(c, hipMemsetAsync(c->kd.slots.p, 0xff, 4 * m, c->stream));
  HIPCHK(c, hipMemsetAsync(c->kd.cnt.p, 0, 4, c->stream));
  TRY(launch(c, c->stream, "kd_insert", grid_lanes(n), k_kd_insert, d_pks, (uint32_t)n, (uint32_t*)c->kd.slots.p, (uint32_t)(m - 1), c->kd.seed, (uint32_t*)c->kd.rep.p));
  return launch(c, c->stream, "kd_assign", grid_lanes(n), k_kd_assign, (const uint32_t*)c->kd.rep.p, (uint32_t)n, (uint32_t*)c->kd.kid.p, (uint32_t*)c->kd.cnt.p, (uint32_t*)c->kd.keys.p);
}
// ... and *u_out = the number of distinct keys, read back (one 4-byte copy and a stream synchronisation)
int dedup_keys(blsbn254_ctx* c, const uint8_t* d_pks, size_t n, size_t* u_out) {
  int rc = dedup_enqueue(c, d_pks, n);
  if (rc) return rc;
  uint32_t u = 0;
  TRY(download(c, &u, c->kd.cnt.p, 4));
  *u_out = u;
  return 0;
}
// Behind dedup_enqueue / dedup_keys: the prepared-key pipeline of a chunk enqueued for `cap` distinct keys (d_u: see prepare_keys)
static int verify_deduped_dev(blsbn254_ctx* c, const uint8_t* d_pks, const uint8_t* d_msgs, const uint64_t* d_off, const uint8_t* d_sigs, size_t n, size_t cap,
                              const uint32_t* d_u, uint32_t dl, uint8_t* d_bitmap) {
  KeyTables kt;
  TRY(prepare_keys(c, d_pks, cap, d_u, &kt));
  TRY(dedup_key_ids(c, n, cap, true));
  return verify_prepared_dev(c, kt, cap, (const uint32_t*)c->kd.kid.p, true, d_msgs, d_off, d_sigs, n, dl, d_bitmap);
}
// the exact per-tuple path: every tuple validates its own key and runs the two-pair Miller loop with a variable-Q pair
int verify_exact_dev(blsbn254_ctx* c, const uint8_t* d_pks, const uint8_t* d_msgs, const uint64_t* d_off,
                            const uint8_t* d_sigs, size_t n, uint32_t dl, uint8_t* d_bitmap) {
  ++c->prep.stat[1];
  HIPCHK(c, c->h_ws.reserve(n * 18 * 4)); HIPCHK(c, c->f_ws.reserve(n * 108 * 4));
  HIPCHK(c, c->flags.reserve(n)); HIPCHK(c, c->sub_ok.reserve(n));
  TRY(launch_hash_to_g1(c, c->stream, d_msgs, d_off, n, dl, (int32_t*)c->h_ws.p, n, (uint8_t*)nullptr, 0));
  TRY(launch(c, c->stream, "g2_check", grid_lanes(n), k_g2_check, d_pks, n, (uint8_t*)c->sub_ok.p, (uint8_t*)nullptr));
  TRY(launch(c, c->stream, "miller_verify", grid_lanes(n), k_miller_verify, d_pks, d_sigs, (const int32_t*)c->h_ws.p, n, (int32_t*)c->f_ws.p, (uint8_t*)c->flags.p));
  return run_final_exp(c, (int32_t*)c->f_ws.p, n, n, 0, (const uint8_t*)c->flags.p, (const uint8_t*)c->sub_ok.p, d_bitmap, nullptr, nullptr);
}
// One launch chunk.  Workspace is ~7.4 KB per tuple (H, f, six final-exponentiation phase buffers, ten chain slots); batches
// larger than ctx->chunk (4 Mi) tuples are processed chunk by chunk so that any n fits the 288 GB of HBM.
int verify_chunk_dev(blsbn254_ctx* c, const uint8_t* d_pks, const uint8_t* d_msgs, const uint64_t* d_off,
                            const uint8_t* d_sigs, size_t n, uint32_t dl, uint8_t* d_bitmap) {
  Stream2Guard s2_guard(c);
  // Few distinct keys (a validator set signing many messages): every distinct key is validated and turned into its line
  // table ONCE (G2Prepared), beside hash-to-G1, and the tuples run the table-only Miller loop in key-sorted order.
  // Same bitmap as the exact per-tuple path below, which batches of mostly distinct keys keep taking.
  // Small chunks take it whatever their keys: the wave and quad forms need the tables too (launch_forms.h small_for_prepared).
  const bool small = small_for_prepared(c->forms, n, true);
  if (c->auto_prepare && (n >= 1024 || small)) {
    size_t u = 0;
    int rc = dedup_keys(c, d_pks, n, &u);
    if (rc) return rc;
    if ((u * 2 <= n || small) && u <= PREP_MAX_KEYS) {
      ++c->prep.stat[0];
      c->vq.u_hint = u ? u : 1;
      if (u > c->vq.u_max_seen) c->vq.u_max_seen = u;
      return verify_deduped_dev(c, d_pks, d_msgs, d_off, d_sigs, n, u, nullptr, dl, d_bitmap);
    }
  }
  c->vq.u_hint = 0;                                      // keys did not repeat: the next call counts them first again
  return verify_exact_dev(c, d_pks, d_msgs, d_off, d_sigs, n, dl, d_bitmap);
}
// The key capacity a chunk of n tuples would be enqueued with, or 0 when it has to take the counting path.  Host state only: the
// caller decides with it BEFORE it stages its tag (see verify_batch_dev_impl).
static size_t async_capacity(const blsbn254_ctx* c, size_t n, size_t dst_len) {
  const bool small = small_for_prepared(c->forms, n, true);
  if (!c->vq.async || !c->auto_prepare || c->vq.u_hint == 0 || !(n >= 1024 || small) || dst_len > 255) return 0;
  size_t cap = 2 * c->vq.u_hint < 1024 ? 1024 : 2 * c->vq.u_hint;
  if (cap < c->vq.u_max_seen) cap = c->vq.u_max_seen;
  if (cap > PREP_MAX_KEYS) cap = PREP_MAX_KEYS;
  if (cap > n) cap = n;
  if (!small && cap > n / 2) cap = n / 2;
  return cap;
}
// ---- asynchronous variant: no read-back before the pipeline is enqueued.
// A steady caller's batches repeat their key set: after a chunk has taken the prepared-key path, the NEXT chunk is enqueued on the
// assumption that it does too, with tables reserved for twice the last key count -- de-duplication, a one-lane decision kernel
// (key count <= capacity, and at most half of the keys distinct unless the chunk is small), the per-key preparation bounded by
// the DEVICE-side count, the table-only pipeline -- and the call returns.  Count and decision come back through a pinned
// buffer behind an event; they are read by the next entry point that touches the context (ENTER) or by
// blsbn254_ctx_synchronize.  If the assumption did not hold (a new key set, more keys than reserved), that batch's bitmap is
// not valid yet: it is re-run on the counting path right there, before the caller can see it -- key ids beyond the capacity were
// clamped by k_kd_propagate, so the discarded run indexed nothing out of bounds.  The caller's device buffers must stay untouched
// until blsbn254_ctx_synchronize returns, as the header has always required of the device entry points.
// The caller has made room in the queue (fewer than four calls pending) and staged the tag; nothing in here settles a pending call.
static int verify_chunk_async(blsbn254_ctx* c, const uint8_t* d_pks, const uint8_t* d_msgs, const uint64_t* d_off, const uint8_t* d_sigs, size_t n,
                              size_t cap, uint32_t dl, const uint8_t* dst, size_t dst_len, uint8_t* d_bitmap) {
  const bool small = small_for_prepared(c->forms, n, true);
  if (cap == 0 || c->vq.count >= 4) { c->last_error = "verify_chunk_async: not eligible or queue full"; return BLSBN254_E_ARG; }
  if (!c->vq.host) {
    HIPCHK(c, hipHostMalloc((void**)&c->vq.host, 4 * 2 * sizeof(uint32_t), hipHostMallocDefault));
    HIPCHK(c, c->vq.dev.reserve(4 * 2 * sizeof(uint32_t)));
    for (auto& pv : c->vq.pend) HIPCHK(c, hipEventCreateWithFlags(&pv.ev, hipEventDisableTiming));
  }
  Stream2Guard s2_guard(c);
  const int slot = (c->vq.head + c->vq.count) & 3;
  uint32_t* d_res = (uint32_t*)c->vq.dev.p + 2 * slot;
  TRY(dedup_enqueue(c, d_pks, n));
  TRY(launch(c, c->stream, nullptr, Shape{dim3(1), dim3(1)}, k_kd_decide, (const uint32_t*)c->kd.cnt.p, (uint32_t)n, (uint32_t)cap, small ? 1 : 0, d_res));
  TRY(verify_deduped_dev(c, d_pks, d_msgs, d_off, d_sigs, n, cap, d_res, dl, d_bitmap));   // (d_res[0]: the key count k_kd_decide left)
  PendingVerify& pv = c->vq.pend[slot];
  HIPCHK(c, hipMemcpyAsync(c->vq.host + 2 * slot, d_res, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipEventRecord(pv.ev, c->stream));
  pv.d_pks = d_pks; pv.d_msgs = d_msgs; pv.d_off = d_off; pv.d_sigs = d_sigs; pv.n = n; pv.d_bitmap = d_bitmap;
  pv.dst_len = dst_len;
  if (dst_len) std::memcpy(pv.dst, dst, dst_len);
  ++c->vq.count;
  ++c->vq.stat[0];
  return 0;
}
// Read back the checks of the asynchronously enqueued chunks, oldest first (blocking: all of them; else only those whose event has
// fired); a chunk whose optimistic choice did not hold is re-run on the counting path.
int resolve_pending(blsbn254_ctx* c, bool blocking) {
  while (c->vq.count) {
    PendingVerify& pv = c->vq.pend[c->vq.head];
    if (!blocking && hipEventQuery(pv.ev) != hipSuccess) { (void)hipGetLastError(); break; }
    HIPCHK(c, hipEventSynchronize(pv.ev));
    const uint32_t u = c->vq.host[2 * c->vq.head], ok = c->vq.host[2 * c->vq.head + 1];
    const PendingVerify done = pv;
    c->vq.head = (c->vq.head + 1) & 3; --c->vq.count;
    if (ok) { c->vq.u_hint = u ? u : 1; if (u > c->vq.u_max_seen) c->vq.u_max_seen = u; ++c->prep.stat[0]; continue; }
    ++c->vq.stat[1];
    c->vq.u_hint = 0;
    uint32_t dl; int rc = stage_dst(c, done.dst, done.dst_len, &dl);
    if (rc) return rc;
    rc = verify_chunk_dev(c, done.d_pks, done.d_msgs, done.d_off, done.d_sigs, done.n, dl, done.d_bitmap);
    if (rc) return rc;
  }
  return 0;
}
static int verify_batch_dev_impl(blsbn254_ctx* c, const uint8_t* d_pks, const uint8_t* d_msgs, const uint64_t* d_off,
                                 const uint8_t* d_sigs, size_t n, const uint8_t* dst, size_t dst_len, uint8_t* d_bitmap, bool allow_async) {
  if (!c || (n && (!d_pks || !d_off || !d_sigs || !d_bitmap)) || (dst_len && !dst)) return BLSBN254_E_ARG;
  if (n == 0) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  int rc = resolve_pending(c, !allow_async);           // settle what has already come back (everything, for a caller that reads the result right away)
  if (rc) return rc;
  // Everything that can still re-run an older call is settled BEFORE this call's tag is staged: a re-run stages the older
  // call's tag, and one that ran between stage_dst and the kernels below would leave them hashing under the wrong tag.  The
  // path is chosen from host state alone (no read-back); the queue is drained when it is full or when this call takes the
  // counting path, which reads back anyway.
  const size_t cap = (allow_async && n <= c->chunk) ? async_capacity(c, n, dst_len) : 0;
  if (c->vq.count && (cap == 0 || c->vq.count == 4)) { rc = resolve_pending(c, true); if (rc) return rc; }
  uint32_t dl; rc = stage_dst(c, dst, dst_len, &dl);   // (a new tag waits for the kernels that still read the old one)
  if (rc) return rc;
  if (cap) return verify_chunk_async(c, d_pks, d_msgs, d_off, d_sigs, n, cap, dl, dst, dst_len, d_bitmap);
  return for_chunks(c, n, [&](size_t lo, size_t m) {
    return verify_chunk_dev(c, d_pks + 128 * lo, d_msgs, d_off + lo, d_sigs + 64 * lo, m, dl, d_bitmap + lo / 8);
  });
}
int blsbn254_verify_batch_dev(blsbn254_ctx* c, const uint8_t* d_pks, const uint8_t* d_msgs, const uint64_t* d_off,
                              const uint8_t* d_sigs, size_t n, const uint8_t* dst, size_t dst_len, uint8_t* d_bitmap) {
  return verify_batch_dev_impl(c, d_pks, d_msgs, d_off, d_sigs, n, dst, dst_len, d_bitmap, true);
}
// for callers inside the library that consume the bitmap on the stream right behind the call (host-pointer entry points, the
// multi-device handle): the counting path, nothing left pending
int blsbn254_internal_verify_batch_dev_sync(blsbn254_ctx* c, const uint8_t* d_pks, const uint8_t* d_msgs, const uint64_t* d_off,
                                            const uint8_t* d_sigs, size_t n, const uint8_t* dst, size_t dst_len, uint8_t* d_bitmap) {
  return verify_batch_dev_impl(c, d_pks, d_msgs, d_off, d_sigs, n, dst, dst_len, d_bitmap, false);
}
int blsbn254_async_stats(blsbn254_ctx* c, uint64_t out[2]) { return COPY_STATS(c, vq.stat, 2, out); }
// The store's size in keys (0: no store -- every call prepares its keys, the kernels and arguments of a build without one).
// Settles what is pending, waits for the device and empties the store; its memory is taken by the next call that uses it.
int blsbn254_set_key_cache(blsbn254_ctx* c, size_t max_keys) {
  if (!c || max_keys > PREP_MAX_KEYS) return BLSBN254_E_ARG;
  ENTER(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->kc.max = max_keys; c->kc.cap = 0;
  return 0;
}
// out: keys found resident, keys prepared, times the store was emptied because a batch did not fit behind the resident keys
// (all three counted on the device, over every enqueued run, a discarded one included), keys resident now.  Waits for the device.
int blsbn254_key_cache_stats(blsbn254_ctx* c, uint64_t out[4]) {
  if (!c || !out) return BLSBN254_E_ARG;
  out[0] = out[1] = out[2] = out[3] = 0;
  ENTER(c);
  if (!c->kc.state.p) return 0;
  uint64_t h[7];
  TRY(download(c, h, c->kc.state.p, sizeof h));
  out[0] = h[4 + KC_STAT_HITS]; out[1] = h[4 + KC_STAT_MISSES]; out[2] = h[4 + KC_STAT_RESETS];
  out[3] = c->kc.cap ? (uint32_t)(h[KC_COUNT / 2] >> (32 * (KC_COUNT % 2))) : 0;
  return 0;
}
int blsbn254_set_async_verify(blsbn254_ctx* c, int on) {
  if (!c) return BLSBN254_E_ARG;
  ENTER(c);
  c->vq.async = on != 0;
  return 0;
}
// ---------------- G2Prepared: explicit API
int blsbn254_g2_prepare_batch(blsbn254_ctx* c, const uint8_t* pks, size_t u, blsbn254_g2prepared** out) {
  if (!c || !out || (u && !pks)) return BLSBN254_E_ARG;
  *out = nullptr;
  if (u + 1 > PREP_MAX_KEYS) { c->last_error = "more than 65535 keys in one prepared table"; return BLSBN254_E_ARG; }
  ENTER(c);
  // owned until handed to the caller: every failure path below frees the object and, with it, its three device buffers
  struct Owner { blsbn254_g2prepared* p; ~Owner() { delete p; } } own{new blsbn254_g2prepared()};
  blsbn254_g2prepared* p = own.p;
  p->ctx = c; p->u = u;
  // entry u (one past the caller's keys) is -G2gen: the second member of the aggregate signature's pair
  const size_t u1 = u + 1;
  HIPCHK(c, p->table.reserve(u1 * PREP_KEY_LIMBS * 4)); HIPCHK(c, p->ok.reserve(u1)); HIPCHK(c, c->in_a.reserve(128 * u1)); HIPCHK(c, p->raw.reserve(u1 * PREP_RAW_LIMBS * 4));
  if (u) HIPCHK(c, hipMemcpyAsync(c->in_a.p, pks, 128 * u, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync((uint8_t*)c->in_a.p + 128 * u, NEG_G2_BYTES, 128, hipMemcpyHostToDevice, c->stream));
  TRY(launch_g2_prepare(c, c->stream, (const uint8_t*)c->in_a.p, nullptr, u1, (int32_t*)p->raw.p, (uint8_t*)p->ok.p, nullptr));
  TRY(launch(c, c->stream, "g2_expand", grid_lanes(u1 * (size_t)BN_NEG_G2_LINES), k_g2_expand, (const int32_t*)p->raw.p, (uint32_t)u1, (int32_t*)p->table.p, (const uint32_t*)nullptr, (uint8_t*)p->ok.p));
  hipError_t es = hipStreamSynchronize(c->stream);
  if (es != hipSuccess) { (void)hipDeviceSynchronize(); }       // nothing may still be writing the buffers the owner frees
  HIPCHK(c, es);
  own.p = nullptr;
  *out = p;
  return 0;
}
void blsbn254_g2prepared_destroy(blsbn254_g2prepared* p) {
  if (!p) return;
  (void)hipSetDevice(p->ctx->device);
  (void)hipStreamSynchronize(p->ctx->stream);
  delete p;
}
size_t blsbn254_g2prepared_count(const blsbn254_g2prepared* p) { return p ? p->u : 0; }
// key validity (on curve, not the identity, in the r-torsion) of every prepared key, as a bitmap
int blsbn254_g2prepared_valid(blsbn254_ctx* c, const blsbn254_g2prepared* p, uint8_t* ok_bitmap) {
  if (!c || !p || p->ctx != c || (p->u && !ok_bitmap)) return BLSBN254_E_ARG;
  if (!p->u) return 0;
  ENTER(c);
  HIPCHK(c, c->bitmap.reserve((p->u + 7) / 8 + 8));
  TRY(launch(c, c->stream, "pack_bitmap", grid_lanes(p->u), k_pack_bitmap, (const uint8_t*)p->ok.p, p->u, (uint8_t*)c->bitmap.p));
  return download(c, ok_bitmap, c->bitmap.p, (p->u + 7) / 8);
}
int blsbn254_verify_batch_prepared(blsbn254_ctx* c, const blsbn254_g2prepared* keys, const uint32_t* key_idx, const uint8_t* msgs, const uint64_t* off,
                                   const uint8_t* sigs, size_t n, const uint8_t* dst, size_t dst_len, uint8_t* bm) {
  if (!c || !keys || keys->ctx != c || !off || (n && (!key_idx || !sigs || !bm)) || (dst_len && !dst)) return BLSBN254_E_ARG;
  if (n == 0) return 0;
  ENTER(c);
  uint32_t dl; int rc = stage_dst(c, dst, dst_len, &dl);
  if (rc) return rc;
  rc = stage_msgs(c, msgs, off, n);
  if (rc) return rc;
  const size_t nb = (n + 7) / 8;
  HIPCHK(c, c->bitmap.reserve(nb + 8));
  TRY(upload(c, c->in_b, sigs, 64 * n));
  TRY(upload(c, c->kd.kid, key_idx, 4 * n));
  const KeyTables kt{(const int32_t*)keys->table.p, (const uint8_t*)keys->ok.p, nullptr};
  TRY(for_chunks(c, n, [&](size_t lo, size_t m) {
    return verify_prepared_dev(c, kt, keys->u, (const uint32_t*)c->kd.kid.p + lo, false, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p + lo,
                               (const uint8_t*)c->in_b.p + 64 * lo, m, dl, (uint8_t*)c->bitmap.p + lo / 8);
  }));
  return download(c, bm, c->bitmap.p, nb);
}
// (blsbn254_multi_miller_loop_prepared and blsbn254_aggregate_verify_prepared read the RAW tables: host_aggregate.hip)
// how many verify chunks took the prepared-key path / the exact per-tuple path on this context (tests, bench)
int blsbn254_path_stats(blsbn254_ctx* c, uint64_t out[2]) { return COPY_STATS(c, prep.stat, 2, out); }
int blsbn254_aggregate_path_stats(blsbn254_ctx* c, uint64_t out[2]) { return COPY_STATS(c, agg_stat, 2, out); }
int blsbn254_set_auto_prepare(blsbn254_ctx* c, int on) { if (!c) return BLSBN254_E_ARG; c->auto_prepare = on != 0; return 0; }

int blsbn254_verify_batch(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs,
                          size_t n, const uint8_t* dst, size_t dst_len, uint8_t* bm) {
  if (!c || !off || (n && (!pks || !sigs || !bm)) || (dst_len && !dst)) return BLSBN254_E_ARG;
  if (n == 0) return 0;
  ENTER(c);
  return verify_batch_host(c, pks, msgs, off, sigs, n, dst, dst_len, bm, false);
}
int verify_batch_host(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs, size_t n, const uint8_t* dst,
                      size_t dst_len, uint8_t* bm, bool compressed) {
  int rc = stage_msgs(c, msgs, off, n);
  if (rc) return rc;
  size_t nb = (n + 7) / 8;
  HIPCHK(c, c->bitmap.reserve(nb + 8));
  TRY(stage_g2(c, pks, n, compressed));
  TRY(stage_g1(c, sigs, n, compressed));
  rc = blsbn254_internal_verify_batch_dev_sync(c, (const uint8_t*)c->in_a.p, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p,
                                 (const uint8_t*)c->in_b.p, n, dst, dst_len, (uint8_t*)c->bitmap.p);
  if (rc) return rc;
  return download(c, bm, c->bitmap.p, nb);
}

}  // extern "C"
