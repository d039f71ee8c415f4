// host_rlc.hip -- random-linear-combination batch verification: per-key sums, the chunk / key rounds over
// repeated keys (k_rlc2.hip) and the distinct-key variant (k_rlc.hip).  Host side of include/blsbn254.h; see host_common.h for
// the workspaces (KeySumWs, Rlc2Ws, RlcWs) and rlc_plan.h for what is decided without the device.
#include "host_common.h"

extern "C" {

// ---------------- sums of G1 points per key
// `items` homogeneous points (limb-major at pts, stride pts_stride; optionally a second array pts2 summed alongside) are grouped
// by key in key order: item j has key kid[mark_perm[j]] and is the point in column pt_perm[j] (or j when pt_perm is NULL); key k
// owns hist[k] consecutive items ending at run_end[k].  Level by level, runs are cut into chunks of at most KEY_SUM_GROUP items,
// every chunk is summed by one lane, and the chunk sums (in key order too) are the items of the next level, until every key has
// ONE sum: *out / *out2 (stride u), indexed by key id.  One host synchronisation per level (the chunk count).
static const size_t KEY_SUM_GROUP = 32;
int key_sums(blsbn254_ctx* c, const int32_t* pts, const int32_t* pts2, size_t pts_stride, const uint32_t* mark_perm, const uint32_t* pt_perm,
                    const uint32_t* kid, const uint32_t* hist, const uint32_t* run_end, size_t items, size_t u, const int32_t** out, const int32_t** out2) {
  KeySumWs& w = c->ks;
  const size_t G = KEY_SUM_GROUP, m_max = rlc_chunk_bound(items, G, u);
  const uint32_t u32 = (uint32_t)u, G32 = (uint32_t)G;
  for (int t = 0; t < 2; ++t) {
    HIPCHK(c, w.cnt[t].reserve(4 * (u + 2))); HIPCHK(c, w.base[t].reserve(4 * (u + 2))); HIPCHK(c, w.kid[t].reserve(4 * m_max));
    HIPCHK(c, w.out[t].reserve(27 * 4 * m_max));
    if (pts2) HIPCHK(c, w.out2[t].reserve(27 * 4 * m_max));
  }
  HIPCHK(c, w.start.reserve(4 * m_max)); HIPCHK(c, w.len.reserve(4 * m_max)); HIPCHK(c, w.tchunk.reserve(4 * items)); HIPCHK(c, w.iota.reserve(4 * m_max));
  uint32_t *iota = (uint32_t*)w.iota.p, *tchunk = (uint32_t*)w.tchunk.p, *start = (uint32_t*)w.start.p, *len = (uint32_t*)w.len.p;
  TRY(launch(c, c->stream, "iota", grid_lanes(m_max), k_iota_u32, iota, (uint32_t)m_max));
  int a = 0;
  for (int level = 0; ; ++level) {
    if (level > 8) { c->last_error = "internal: key sums do not converge"; return BLSBN254_E_HIP; }
    uint32_t *cnt = (uint32_t*)w.cnt[a].p, *base = (uint32_t*)w.base[a].p, *ckid = (uint32_t*)w.kid[a].p;
    int32_t *sum = (int32_t*)w.out[a].p, *sum2 = pts2 ? (int32_t*)w.out2[a].p : nullptr;
    TRY(launch(c, c->stream, "rlc2_counts", grid_lanes(u + 1), k_rlc2_chunk_counts, hist, u32, G32, cnt));
    TRY(launch(c, c->stream, "kd_scan", Shape{dim3(1), dim3(1024)}, k_scan_excl, cnt, u32 + 1, base));
    w.h_m = 0;
    TRY(download(c, &w.h_m, base + u, 4));
    const size_t m = w.h_m;
    if (!rlc_level_in_range(m, u, m_max, items)) { c->last_error = "internal: chunk count out of range"; return BLSBN254_E_HIP; }
    TRY(launch(c, c->stream, "rlc2_mark", grid_lanes(items), k_rlc2_mark, mark_perm, kid, hist, run_end, base, (uint32_t)items, G32,
               tchunk, ckid, start, len));
    TRY(launch(c, c->stream, "g1_seg_sum", grid_lanes(m), k_g1_seg_sum, pts, pts_stride, pt_perm, start, len, m, sum, m));
    if (pts2) TRY(launch(c, c->stream, "g1_seg_sum", grid_lanes(m), k_g1_seg_sum, pts2, pts_stride, pt_perm, start, len, m, sum2, m));
    pts = sum; pts2 = sum2; pts_stride = m; items = m;
    if (m == u) break;                                                          // one chunk per key: chunk index == key id
    // next level: item j has key ckid[j]; key k owns items base[k] .. base[k + 1]
    mark_perm = iota; pt_perm = nullptr; kid = ckid; hist = cnt; run_end = base + 1;
    a ^= 1;
  }
  *out = pts;
  if (out2) *out2 = pts2;
  return 0;
}

// ---------------- random-linear-combination batch verification over repeated keys (k_rlc2.hip)
int stage_seed(blsbn254_ctx* c, DevBuf& d, const uint8_t* seed) {
  uint8_t* h_seed = c->r2.h_seed;
  if (seed) std::memcpy(h_seed, seed, 32);
  for (size_t got = 0; !seed && got < 32; ) {          // the normal case: 32 bytes from the OS, drawn now -- after the batch is fixed
    ssize_t k = getrandom(h_seed + got, 32 - got, 0);
    if (k <= 0) { c->last_error = "getrandom failed"; return BLSBN254_E_HIP; }
    got += (size_t)k;
  }
  return upload(c, d, h_seed, 32);
}
// One table-only Miller loop + final exponentiation over `cnt` (virtual or real) tuples: is_one bytes to d_isone, flags in ctx->flags.
// kid[perm[s]] names the key's entry in kt's tables: what miller_ids / key_miller_ids make of the batch key ids.
int prepared_round(blsbn254_ctx* c, const uint32_t* perm, const uint32_t* kid, const KeyTables& kt, const uint8_t* sigs, const int32_t* h_ws, size_t h_stride, size_t cnt, uint8_t* d_isone) {
  HIPCHK(c, c->f_ws.reserve(cnt * 108 * 4)); HIPCHK(c, c->flags.reserve(cnt));
  TRY(launch_miller_prepared(c, perm, kid, sigs, h_ws, h_stride, kt, cnt));
  return run_final_exp(c, (int32_t*)c->f_ws.p, cnt, cnt, 4, nullptr, nullptr, nullptr, d_isone, nullptr);
}
// One call of rlc2_chunk_dev as its stages see it: the sizes, the key-sorted order and the batch key id per tuple, the validity
// bytes by batch key id, the Miller loops' key ids of tuples and of chunks, the key tables; what the key round leaves for the
// chunk round: the chunks to check (NULL: all m, in order) and their number.  Everything else is in c->r2.
struct Rlc2Call {
  size_t n, u, m, G;
  const uint32_t *perm, *kid;
  const uint8_t* key_ok;
  const uint32_t *tuple_slot, *chunk_slot;
  KeyTables kt;
  const uint32_t* clist; size_t mc;
};
// The weights: the keys' tables on the second stream, key ids and key-sorted order, the chunk numbering, the hash points and the
// weighted points r_i sig_i, r_i H_i, their sums per chunk; joined with the key tables.  Fills q.m and everything behind it.
static int rlc2_weigh(blsbn254_ctx* c, Rlc2Call& q, const uint8_t* d_pks, const uint8_t* d_msgs, const uint64_t* d_off, const uint8_t* d_sigs, uint32_t dl,
                      const uint8_t* d_seed) {
  Rlc2Ws& w = c->r2;
  const size_t n = q.n, u = q.u, nblk = (n + 255) / 256;
  const uint32_t G32 = (uint32_t)q.G, n32 = (uint32_t)n, u32 = (uint32_t)u;
  // The keys' tables, on the second stream (with a store of prepared keys only the keys new to it are prepared: the Miller loops
  // take miller_ids where they take key ids, the other kernels keys_valid's bytes in batch key order)
  TRY(prepare_keys(c, d_pks, u, nullptr, &q.kt));
  HIPCHK(c, c->h_ws.reserve(n * 27 * 4)); HIPCHK(c, w.a.reserve(n * 27 * 4)); HIPCHK(c, w.b.reserve(n * 27 * 4)); HIPCHK(c, w.sigok.reserve(n));
  HIPCHK(c, w.tchunk.reserve(4 * n)); HIPCHK(c, w.ccnt.reserve(4 * (u + 2))); HIPCHK(c, w.cbase.reserve(4 * (u + 2)));
  HIPCHK(c, w.need.reserve(n)); HIPCHK(c, w.bcnt.reserve(4 * (nblk + 2))); HIPCHK(c, w.bbase.reserve(4 * (nblk + 2)));
  HIPCHK(c, w.list.reserve(4 * n)); HIPCHK(c, w.valid.reserve(n));
  const uint32_t *hist = (const uint32_t*)c->kd.hist.p, *kid = (const uint32_t*)c->kd.kid.p;
  uint32_t *ccnt = (uint32_t*)w.ccnt.p, *cbase = (uint32_t*)w.cbase.p, *tchunk = (uint32_t*)w.tchunk.p;
  int32_t *h = (int32_t*)c->h_ws.p, *wa = (int32_t*)w.a.p, *wb = (int32_t*)w.b.p;
  uint8_t* sigok = (uint8_t*)w.sigok.p;
  // key ids, key-sorted order, chunk numbering
  TRY(dedup_key_ids(c, n, u, true));
  TRY(key_sorted_order(c, kid, n, u));                 // cursor[k] is now the END of run k
  const uint32_t *cursor = (const uint32_t*)c->kd.cursor.p, *perm = (const uint32_t*)c->kd.perm.p;
  TRY(launch(c, c->stream, "rlc2_counts", grid_lanes(u + 1), k_rlc2_chunk_counts, hist, u32, G32, ccnt));
  TRY(launch(c, c->stream, "kd_scan", Shape{dim3(1), dim3(1024)}, k_scan_excl, ccnt, u32 + 1, cbase));
  w.h_m = 0;
  HIPCHK(c, hipMemcpyAsync(&w.h_m, cbase + u, 4, hipMemcpyDeviceToHost, c->stream));
  // the hash points and the weighted points r_i sig_i, r_i H_i (the host learns the chunk count while these run)
  TRY(launch_hash_to_g1(c, c->stream, d_msgs, d_off, n, dl, h, n, (uint8_t*)nullptr, 3));
  TRY(launch(c, c->stream, "rlc2_prep", grid_lanes(n), k_rlc2_prep, perm, d_pks, d_sigs, h, n, d_seed, wa, wb, sigok));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t m = w.h_m;
  if (!rlc_chunks_in_range(m, n)) { c->last_error = "internal: chunk count out of range"; return BLSBN254_E_HIP; }
  HIPCHK(c, w.ckid.reserve(4 * m)); HIPCHK(c, w.cstart.reserve(4 * m)); HIPCHK(c, w.clen.reserve(4 * m)); HIPCHK(c, w.csig.reserve(64 * m));
  HIPCHK(c, w.ch.reserve(27 * 4 * m)); HIPCHK(c, w.cstate.reserve(m)); HIPCHK(c, w.iota.reserve(4 * m)); HIPCHK(c, w.cisone.reserve(m));
  uint32_t *ckid = (uint32_t*)w.ckid.p, *cstart = (uint32_t*)w.cstart.p, *clen = (uint32_t*)w.clen.p;
  TRY(launch(c, c->stream, "rlc2_mark", grid_lanes(n), k_rlc2_mark, perm, kid, hist, cursor, cbase, n32, G32, tchunk, ckid, cstart, clen));
  HIPCHK(c, w.sa.reserve(27 * 4 * m)); HIPCHK(c, w.sb.reserve(27 * 4 * m)); HIPCHK(c, w.celig.reserve(4 * m));
  TRY(launch(c, c->stream, "rlc2_sum", grid_lanes(m), k_rlc2_sum, wa, wb, n, sigok, cstart, clen, m, (int32_t*)w.sa.p, (int32_t*)w.sb.p, (uint32_t*)w.celig.p));
  HIPCHK(c, join_stream2(c));                      // the key tables are ready
  q.m = m; q.mc = m; q.clist = nullptr; q.perm = perm; q.kid = kid;
  TRY(keys_valid(c, q.kt, u, &q.key_ok));
  TRY(miller_ids(c, q.kt, kid, n, c->kc.tslot, &q.tuple_slot));
  TRY(miller_ids(c, q.kt, ckid, m, c->kc.cslot, &q.chunk_slot));
  // what the rounds share: the chunks' verdicts, the list of those the key round leaves, 0, 1, 2, ... over the chunks
  const size_t mblk = (m + 255) / 256;
  HIPCHK(c, w.cpass.reserve(m)); HIPCHK(c, w.clist.reserve(4 * m)); HIPCHK(c, w.cneed.reserve(m)); HIPCHK(c, w.cbcnt.reserve(4 * (mblk + 2)));
  HIPCHK(c, w.cbbase.reserve(4 * (mblk + 2)));
  return launch(c, c->stream, "iota", grid_lanes(m), k_iota_u32, (uint32_t*)w.iota.p, (uint32_t)m);
}
// The key round: ALL tuples of a key as one virtual tuple (the chunk sums of the key, summed) -- u checks, few enough for the
// wave-per-tuple kernels.  A batch without invalid signatures (the usual case) is decided here, in a fraction of a chunk round
// (*decided: the validity bytes are final); otherwise only the chunks of the keys that failed are left for the chunk round
// (q.clist, q.mc).  Same weights, hence the same 2^-64 bound per check.
static int rlc2_key_round(blsbn254_ctx* c, Rlc2Call& q, bool* decided) {
  Rlc2Ws& w = c->r2;
  const size_t n = q.n, u = q.u, m = q.m, mblk = (m + 255) / 256;
  HIPCHK(c, w.kelig.reserve(4 * u)); HIPCHK(c, w.ksig.reserve(64 * u)); HIPCHK(c, w.kh.reserve(27 * 4 * u)); HIPCHK(c, w.kstate.reserve(u));
  HIPCHK(c, w.kisone.reserve(u)); HIPCHK(c, w.kpass.reserve(u)); HIPCHK(c, c->misc.reserve(64));
  const uint32_t *iota = (const uint32_t*)w.iota.p, *ckid = (const uint32_t*)w.ckid.p, *celig = (const uint32_t*)w.celig.p;
  const uint32_t *ccnt = (const uint32_t*)w.ccnt.p, *cbase = (const uint32_t*)w.cbase.p;
  uint32_t *kelig = (uint32_t*)w.kelig.p, *cbcnt = (uint32_t*)w.cbcnt.p, *cbbase = (uint32_t*)w.cbbase.p, *clist = (uint32_t*)w.clist.p;
  uint8_t *ksig = (uint8_t*)w.ksig.p, *kstate = (uint8_t*)w.kstate.p, *kisone = (uint8_t*)w.kisone.p, *kpass = (uint8_t*)w.kpass.p, *cneed = (uint8_t*)w.cneed.p;
  int32_t* kh = (int32_t*)w.kh.p;
  const int32_t *ksa = nullptr, *ksb = nullptr;
  TRY(key_sums(c, (const int32_t*)w.sa.p, (const int32_t*)w.sb.p, m, iota, nullptr, ckid, ccnt, cbase + 1, m, u, &ksa, &ksb));
  HIPCHK(c, hipMemsetAsync(kelig, 0, 4 * u, c->stream));
  TRY(launch(c, c->stream, "rlc2_key_elig", grid_lanes(m), k_rlc2_key_elig, ckid, celig, (uint32_t)m, kelig));
  TRY(launch(c, c->stream, "rlc2_virtual", grid_lanes(u), k_rlc2_virtual, ksa, ksb, u, kelig, (const uint32_t*)nullptr, u, ksig, kh, kstate));
  TRY(prepared_round(c, iota, key_miller_ids(q.kt, iota), q.kt, ksig, kh, u, u, kisone));
  int* d_all = (int*)c->misc.p;                        // the verdict: 1 until a key fails
  static const int one_i = 1;
  HIPCHK(c, hipMemcpyAsync(d_all, &one_i, 4, hipMemcpyHostToDevice, c->stream));
  TRY(launch(c, c->stream, "rlc2_keys_pass", grid_lanes(u), k_rlc2_keys_pass, q.key_ok, kstate, kisone, (uint32_t)u, kpass, d_all));
  // the chunks of the keys that failed, as an ordered list (counted while the host waits for the verdict)
  TRY(launch(c, c->stream, "rlc2_chunk_need", grid_lanes(m), k_rlc2_chunk_need, ckid, kpass, (uint32_t)m, cneed, cbcnt));
  TRY(launch(c, c->stream, "kd_scan", Shape{dim3(1), dim3(1024)}, k_scan_excl, cbcnt, (uint32_t)mblk + 1, cbbase));
  w.h_all_pass = 0; w.h_mc = 0;
  HIPCHK(c, hipMemcpyAsync(&w.h_all_pass, d_all, 4, hipMemcpyDeviceToHost, c->stream));
  TRY(download(c, &w.h_mc, cbbase + mblk, 4));
  w.stat[0] += n; ++w.stat[4];
  if (w.h_all_pass == 1) {
    ++w.stat[5];
    w.backoff.passed();
    *decided = true;
    return launch(c, c->stream, "rlc2_valid_fast", grid_lanes(n), k_rlc2_valid_fast, q.perm, q.kid, (const uint8_t*)w.sigok.p, q.key_ok, (uint32_t)n, (uint8_t*)w.valid.p);
  }
  w.backoff.failed();
  if (!rlc_list_in_range(w.h_mc, m)) { c->last_error = "internal: chunk list out of range"; return BLSBN254_E_HIP; }
  q.mc = w.h_mc;
  TRY(launch(c, c->stream, "rlc2_compact", grid_lanes(m), k_rlc2_compact, cneed, iota, (uint32_t)m, cbbase, clist));
  q.clist = clist;
  HIPCHK(c, hipMemsetAsync(w.cpass.p, 1, m, c->stream));               // chunks of the keys that passed
  return 0;
}
// The chunk round: every (listed) chunk is one virtual tuple on the prepared-key verify path; then per tuple the verdict its
// chunk leaves, and the count of the eligible tuples of failed chunks (enqueued: the fallback reads it)
static int rlc2_chunk_round(blsbn254_ctx* c, const Rlc2Call& q) {
  Rlc2Ws& w = c->r2;
  const size_t n = q.n, m = q.m, mc = q.mc, nblk = (n + 255) / 256;
  const uint32_t* iota = (const uint32_t*)w.iota.p;
  uint8_t *csig = (uint8_t*)w.csig.p, *cstate = (uint8_t*)w.cstate.p, *cisone = (uint8_t*)w.cisone.p, *cpass = (uint8_t*)w.cpass.p;
  int32_t* ch = (int32_t*)w.ch.p;
  uint32_t *bcnt = (uint32_t*)w.bcnt.p, *bbase = (uint32_t*)w.bbase.p;
  TRY(launch(c, c->stream, "rlc2_virtual", grid_lanes(mc), k_rlc2_virtual, (const int32_t*)w.sa.p, (const int32_t*)w.sb.p, m, (const uint32_t*)w.celig.p, q.clist, mc,
             csig, ch, cstate));
  TRY(prepared_round(c, q.clist ? q.clist : iota, q.chunk_slot, q.kt, csig, ch, m, mc, cisone));
  TRY(launch(c, c->stream, "rlc2_chunk_pass", grid_lanes(mc), k_rlc2_chunk_pass, q.clist, cstate, cisone, (const uint8_t*)c->flags.p, (uint32_t)mc, cpass));
  TRY(launch(c, c->stream, "rlc2_resolve", grid_lanes(n), k_rlc2_resolve, q.perm, q.kid, (const uint32_t*)w.tchunk.p, (const uint8_t*)w.sigok.p, q.key_ok,
             cpass, (uint32_t)n, (uint8_t*)w.valid.p, (uint8_t*)w.need.p, bcnt));
  return launch(c, c->stream, "kd_scan", Shape{dim3(1), dim3(1024)}, k_scan_excl, bcnt, (uint32_t)nblk + 1, bbase);
}
// The fallback: the eligible tuples of failed chunks through the exact prepared-key path, in key-sorted order
static int rlc2_fallback(blsbn254_ctx* c, const Rlc2Call& q, const uint8_t* d_sigs) {
  Rlc2Ws& w = c->r2;
  const size_t n = q.n, nblk = (n + 255) / 256;
  const uint32_t* bbase = (const uint32_t*)w.bbase.p;
  uint32_t* list = (uint32_t*)w.list.p;
  w.h_m2 = 0;
  TRY(download(c, &w.h_m2, bbase + nblk, 4));
  const uint32_t m2 = w.h_m2;
  if (!rlc_fallback_in_range(m2, n)) { c->last_error = "internal: fallback count out of range"; return BLSBN254_E_HIP; }
  w.stat[1] += q.mc; w.stat[2] += m2;
  if (!m2) return 0;
  HIPCHK(c, c->prep.isone.reserve(m2));
  uint8_t* isone = (uint8_t*)c->prep.isone.p;
  TRY(launch(c, c->stream, "rlc2_compact", grid_lanes(n), k_rlc2_compact, (const uint8_t*)w.need.p, q.perm, (uint32_t)n, bbase, list));
  TRY(prepared_round(c, list, q.tuple_slot, q.kt, d_sigs, (const int32_t*)c->h_ws.p, n, m2, isone));
  return launch(c, c->stream, "prep_unsort", grid_lanes(m2), k_prep_unsort, isone, (const uint8_t*)c->flags.p, list, m2, (uint8_t*)w.valid.p);
}
// n <= ctx->chunk tuples, everything device-resident; d_seed = 32 bytes in device memory.  *took = 0 when the keys do not repeat
// (nothing was done: the caller takes another path).
static int rlc2_chunk_dev(blsbn254_ctx* c, const uint8_t* d_pks, const uint8_t* d_msgs, const uint64_t* d_off, const uint8_t* d_sigs, size_t n,
                          uint32_t dl, const uint8_t* d_seed, uint8_t* d_bitmap, bool* took) {
  Stream2Guard s2_guard(c);
  Rlc2Ws& w = c->r2;
  *took = false;
  if (n < 2) return 0;
  Rlc2Call q{};
  q.n = n;
  TRY(dedup_keys(c, d_pks, n, &q.u));
  if (!rlc_keys_repeat(n, q.u, PREP_MAX_KEYS)) return 0;
  *took = true;
  q.G = rlc_chunk_size(n, q.u, w.group, w.group_auto, c->forms);
  TRY(rlc2_weigh(c, q, d_pks, d_msgs, d_off, d_sigs, dl, d_seed));
  bool decided = false;
  if (w.backoff.take(w.key_round)) TRY(rlc2_key_round(c, q, &decided));
  else w.stat[0] += n;
  if (!decided) {
    TRY(rlc2_chunk_round(c, q));
    TRY(rlc2_fallback(c, q, d_sigs));
  }
  return launch(c, c->stream, "pack_bitmap", grid_lanes(n), k_pack_bitmap, (const uint8_t*)w.valid.p, n, d_bitmap);
}
int blsbn254_verify_batch_rlc_dev(blsbn254_ctx* c, const uint8_t* d_pks, const uint8_t* d_msgs, const uint64_t* d_off, const uint8_t* d_sigs, size_t n,
                                  const uint8_t* dst, size_t dst_len, const uint8_t seed[32], uint8_t* d_bitmap) {
  if (!c || (n && (!d_pks || !d_off || !d_sigs || !d_bitmap)) || (dst_len && !dst)) return BLSBN254_E_ARG;
  if (n == 0) return 0;
  ENTER(c);
  uint32_t dl;
  TRY(stage_dst(c, dst, dst_len, &dl));
  TRY(stage_seed(c, c->r2.seed, seed));
  return for_chunks(c, n, [&](size_t lo, size_t m) -> int {
    bool took = false;
    TRY(rlc2_chunk_dev(c, d_pks + 128 * lo, d_msgs, d_off + lo, d_sigs + 64 * lo, m, dl, (const uint8_t*)c->r2.seed.p, d_bitmap + lo / 8, &took));
    if (took) return 0;
    c->r2.stat[3] += m;                                // keys do not repeat: nothing to share per key, the exact per-tuple path
    return verify_exact_dev(c, d_pks + 128 * lo, d_msgs, d_off + lo, d_sigs + 64 * lo, m, dl, d_bitmap + lo / 8);
  });
}
int blsbn254_set_rlc_group(blsbn254_ctx* c, size_t group) {
  if (!c || group == 1 || group > RLC_MAX_GROUP) return BLSBN254_E_ARG;
  c->r2.group = group ? group : RLC_DEFAULT_GROUP;
  c->r2.group_auto = group == 0;
  return 0;
}
int blsbn254_rlc_stats(blsbn254_ctx* c, uint64_t out[6]) { return COPY_STATS(c, r2.stat, 6, out); }
int blsbn254_set_rlc_key_round(blsbn254_ctx* c, int on) { if (!c) return BLSBN254_E_ARG; c->r2.key_round = on != 0; c->r2.backoff.reset(); return 0; }

// ---------------- random-linear-combination batch verification: the distinct-key variant (k_rlc.hip)
static const size_t RLC_GROUP = 16;      // tuples per shared final exponentiation (power of two)
// The group products: groups of RLC_GROUP tuples in the caller's order (the staged batch: c->in_a, in_b, in_c / in_off) share
// the signature-side Miller loop and the final exponentiation.  The bits of the groups that pass into bm; the eligible tuples of
// the others into c->rlc.h_idx.
static int rlc_group_products(blsbn254_ctx* c, size_t n, uint32_t dl, uint8_t* bm) {
  RlcWs& w = c->rlc;
  const size_t G = RLC_GROUP, n_pad = (n + G - 1) / G * G, ng = n_pad / G, nb = (n + 7) / 8;
  HIPCHK(c, c->misc.reserve(64));
  HIPCHK(c, c->h_ws.reserve(n * 18 * 4)); HIPCHK(c, c->sub_ok.reserve(n)); HIPCHK(c, c->flags.reserve(n_pad));
  HIPCHK(c, w.a.reserve(n_pad * 27 * 4)); HIPCHK(c, w.b.reserve(n_pad * 18 * 4)); HIPCHK(c, w.elig.reserve(n_pad));
  HIPCHK(c, c->f_ws.reserve(n_pad * 108 * 4)); HIPCHK(c, w.f2.reserve(ng * 108 * 4)); HIPCHK(c, w.bytes.reserve(ng * 64));
  HIPCHK(c, w.neg.reserve(ng * 128)); HIPCHK(c, w.ok.reserve(ng)); HIPCHK(c, c->status.reserve(ng + 8));
  const uint8_t *d_pks = (const uint8_t*)c->in_a.p, *d_sigs = (const uint8_t*)c->in_b.p;
  int32_t *h = (int32_t*)c->h_ws.p, *f = (int32_t*)c->f_ws.p, *f2 = (int32_t*)w.f2.p, *wa = (int32_t*)w.a.p, *wb = (int32_t*)w.b.p;
  uint8_t *sub_ok = (uint8_t*)c->sub_ok.p, *elig = (uint8_t*)w.elig.p, *bytes = (uint8_t*)w.bytes.p, *neg = (uint8_t*)w.neg.p, *ok = (uint8_t*)w.ok.p;
  HIPCHK(c, hipMemcpyAsync(c->misc.p, c->r2.seed.p, 32, hipMemcpyDeviceToDevice, c->stream));
  w.h_neg.resize(ng * 128);                            // context-owned: the copy needs no wait
  for (size_t g = 0; g < ng; ++g) std::memcpy(w.h_neg.data() + 128 * g, NEG_G2_BYTES, 128);
  HIPCHK(c, hipMemcpyAsync(neg, w.h_neg.data(), ng * 128, hipMemcpyHostToDevice, c->stream));
  TRY(launch_hash_to_g1(c, c->stream, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, n, dl, h, n, (uint8_t*)nullptr, 0));
  TRY(launch(c, c->stream, "g2_check", grid_lanes(n), k_g2_check, d_pks, n, sub_ok, (uint8_t*)nullptr));
  TRY(launch(c, c->stream, "rlc_prep", grid_lanes(n_pad), k_rlc_prep, d_pks, d_sigs, h, sub_ok, (const uint8_t*)c->misc.p, n, n_pad,
             wa, wb, elig));
  // prod_i ML(r_i H_i, pk_i) per group: per-pair loops, ONE where not eligible, log2(G) levels of pairwise products
  TRY(launch(c, c->stream, "miller_hpk", grid_lanes(n), k_miller_hpk, wb, d_pks, n, f, n_pad, (uint8_t*)c->flags.p));
  TRY(launch(c, c->stream, "fp12_mask_one", grid_lanes(n_pad), k_fp12_mask_one, f, n_pad, elig, n_pad));
  HIPCHK(c, c->f_ws2.reserve((n_pad / 2) * 108 * 4)); HIPCHK(c, w.a2.reserve((n_pad / 2) * 27 * 4));
  int32_t *pa = f, *pb = (int32_t*)c->f_ws2.p, *ga = wa, *gb = (int32_t*)w.a2.p;
  size_t cnt = n_pad, st = n_pad;
  for (size_t lvl = 1; lvl < G; lvl <<= 1) {                          // adjacent pairs never straddle a group
    size_t mo = cnt / 2;
    TRY(launch(c, c->stream, "fp12_mul_pairs", grid_lanes(mo), k_fp12_mul_pairs, pa, cnt, st, pb, mo));
    TRY(launch(c, c->stream, "g1_add_pairs", grid_lanes(mo), k_g1_add_pairs, ga, cnt, st, gb, mo));
    std::swap(pa, pb); std::swap(ga, gb); st = mo; cnt = mo;
  }
  // e(sum_i r_i sig_i, -G2gen) per group, multiplied in; one final exponentiation per group
  TRY(launch(c, c->stream, "g1p_to_bytes", grid_lanes(ng), k_g1p_to_bytes, ga, st, ng, bytes));
  TRY(launch(c, c->stream, "miller_1", grid_lanes(ng), k_miller_1, bytes, neg, ng, f2, ng, (uint8_t*)c->status.p));
  TRY(launch(c, c->stream, "fp12_mul_elem", grid_lanes(ng), k_fp12_mul_elem, pa, st, f2, ng, ng));
  TRY(run_final_exp(c, pa, ng, st, 4, nullptr, nullptr, nullptr, ok, nullptr));
  w.h_ok.resize(ng); w.h_elig.resize(n_pad);
  HIPCHK(c, hipMemcpyAsync(w.h_ok.data(), ok, ng, hipMemcpyDeviceToHost, c->stream));
  TRY(download(c, w.h_elig.data(), elig, n_pad));
  std::memset(bm, 0, nb);
  w.h_idx.clear();
  for (size_t g = 0; g < ng; ++g) {
    for (size_t i = g * G; i < (g + 1) * G && i < n; ++i) {
      if (!w.h_elig[i]) continue;                                      // failed a precheck: invalid, not part of any product
      if (w.h_ok[g]) set_bit(bm, i);
      else w.h_idx.push_back((uint32_t)i);
    }
  }
  return 0;
}
// ... and the exact per-tuple path for the tuples c->rlc.h_idx names (the eligible tuples of the groups that failed), one
// sub-call: gathered, verified, their bits merged into bm
static int rlc_exact_failed(blsbn254_ctx* c, size_t n, uint8_t* bm) {
  RlcWs& w = c->rlc;
  if (w.h_idx.empty()) return 0;
  const size_t m = w.h_idx.size(), mb = (m + 7) / 8;
  HIPCHK(c, w.cpk.reserve(128 * m)); HIPCHK(c, w.csig.reserve(64 * m));
  HIPCHK(c, w.ch.reserve(18 * 4 * m)); HIPCHK(c, w.csub.reserve(m)); HIPCHK(c, w.cbm.reserve(mb + 8));
  HIPCHK(c, c->f_ws.reserve(m * 108 * 4)); HIPCHK(c, c->flags.reserve(m));
  TRY(upload(c, w.idx, w.h_idx.data(), 4 * m));
  uint8_t *cpk = (uint8_t*)w.cpk.p, *csig = (uint8_t*)w.csig.p, *csub = (uint8_t*)w.csub.p, *cbm = (uint8_t*)w.cbm.p, *flags = (uint8_t*)c->flags.p;
  int32_t *ch = (int32_t*)w.ch.p, *f = (int32_t*)c->f_ws.p;
  TRY(launch(c, c->stream, "rlc_gather", grid_lanes(m), k_rlc_gather, (const uint32_t*)w.idx.p, m, (const uint8_t*)c->in_a.p, (const uint8_t*)c->in_b.p,
             (const int32_t*)c->h_ws.p, n, (const uint8_t*)c->sub_ok.p, cpk, csig, ch, csub));
  TRY(launch(c, c->stream, "miller_verify", grid_lanes(m), k_miller_verify, cpk, csig, ch, m, f, flags));
  TRY(run_final_exp(c, f, m, m, 0, flags, csub, cbm, nullptr, nullptr));
  w.h_bits.resize(mb);
  TRY(download(c, w.h_bits.data(), cbm, mb));
  for (size_t j = 0; j < m; ++j) if (bit_at(w.h_bits.data(), j)) set_bit(bm, w.h_idx[j]);
  return 0;
}
int blsbn254_verify_batch_rlc(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs,
                              size_t n, const uint8_t* dst, size_t dst_len, const uint8_t seed[32], uint8_t* bm) {
  if (!c || !off || (n && (!pks || !sigs || !bm)) || (dst_len && !dst)) return BLSBN254_E_ARG;
  if (n == 0) return 0;
  ENTER(c);
  return verify_batch_rlc_host(c, pks, msgs, off, sigs, n, dst, dst_len, seed, bm, false);
}
// stage, choose, download
int verify_batch_rlc_host(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs, size_t n, const uint8_t* dst,
                          size_t dst_len, const uint8_t* seed, uint8_t* bm, bool compressed) {
  uint32_t dl;
  TRY(stage_dst(c, dst, dst_len, &dl));
  TRY(stage_msgs(c, msgs, off, n));
  const size_t nb = (n + 7) / 8;
  HIPCHK(c, c->bitmap.reserve(nb + 8));
  TRY(stage_g2(c, pks, n, compressed));
  TRY(stage_g1(c, sigs, n, compressed));
  const uint8_t *d_pks = (const uint8_t*)c->in_a.p, *d_msgs = (const uint8_t*)c->in_c.p, *d_sigs = (const uint8_t*)c->in_b.p;
  const uint64_t* d_off = (const uint64_t*)c->in_off.p;
  uint8_t* d_bitmap = (uint8_t*)c->bitmap.p;
  // Repeated keys: per-key chunks as virtual tuples on the prepared-key path (k_rlc2.hip).  Batches beyond one launch chunk
  // go chunk by chunk through the device entry point (which takes the exact path for a chunk of distinct keys).
  bool took = false;
  if (n <= c->chunk) {
    TRY(stage_seed(c, c->r2.seed, seed));
    TRY(rlc2_chunk_dev(c, d_pks, d_msgs, d_off, d_sigs, n, dl, (const uint8_t*)c->r2.seed.p, d_bitmap, &took));
  } else {                                                               // (the device entry point stages the seed itself)
    TRY(blsbn254_verify_batch_rlc_dev(c, d_pks, d_msgs, d_off, d_sigs, n, dst, dst_len, seed, d_bitmap));
    took = true;
  }
  if (took) return download(c, bm, d_bitmap, nb);
  // Distinct keys: the group products, then the exact path for the groups that failed
  c->r2.stat[3] += n;
  TRY(rlc_group_products(c, n, dl, bm));
  return rlc_exact_failed(c, n, bm);
}

}  // extern "C"
