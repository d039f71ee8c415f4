// host_groupops.hip -- group operations on caller-supplied points and FastAggregateVerify: Mul<Scalar> for G1 / G2,
// impl Sum for G2Projective (aggregate public keys), and "one message signed by many keys" verified as one pairing equation
// per group over the sum of the group's keys.  Host side of include/blsbn254.h; kernels in k_groupops.hip; see host_common.h.
#include "host_common.h"

extern "C" {

// out_i = [k_i] P_i
static int mul_common(blsbn254_ctx* c, const uint8_t* pts, const uint8_t* scalars, size_t n, uint8_t* out, int g2) {
  if (!c || (n && (!pts || !scalars || !out))) return BLSBN254_E_ARG;
  if (n == 0) return 0;
  ENTER(c);
  const size_t sz = g2 ? 128 : 64;
  return for_chunks(c, n, [&](size_t lo, size_t m) -> int {
    HIPCHK(c, c->out.reserve(sz * m)); HIPCHK(c, c->status.reserve(m));
    TRY(upload(c, c->in_a, pts + sz * lo, sz * m));
    TRY(upload(c, c->scalars, scalars + 32 * lo, 32 * m));
    if (g2) TRY(launch(c, c->stream, "g2_mul", grid_lanes(m), k_g2_mul, (const uint8_t*)c->in_a.p, (const uint8_t*)c->scalars.p, m, (uint8_t*)c->out.p, (uint8_t*)c->status.p));
    else TRY(launch(c, c->stream, "g1_mul", grid_lanes(m), k_g1_mul, (const uint8_t*)c->in_a.p, (const uint8_t*)c->scalars.p, m, (uint8_t*)c->out.p, (uint8_t*)c->status.p));
    int bad;
    TRY(first_bad(c, (const uint8_t*)c->status.p, m, 3, 3, &bad));
    if (bad >= 0) {
      uint8_t st = 0;
      TRY(read_status(c, (const uint8_t*)c->status.p, bad, &st));
      c->last_error = std::string(st & 1 ? "scalar not canonical" : "point does not decode or is off the curve") + " at element " + std::to_string(lo + (size_t)bad);
      return (st & 1) ? BLSBN254_ERR_SCALAR : (g2 ? BLSBN254_ERR_G2 : BLSBN254_ERR_G1);
    }
    return download(c, out + sz * lo, c->out.p, sz * m);
  });
}
int blsbn254_g1_mul_batch(blsbn254_ctx* c, const uint8_t* g1, const uint8_t* scalars, size_t n, uint8_t* out) { return mul_common(c, g1, scalars, n, out, 0); }
int blsbn254_g2_mul_batch(blsbn254_ctx* c, const uint8_t* g2, const uint8_t* scalars, size_t n, uint8_t* out) { return mul_common(c, g2, scalars, n, out, 1); }

int plan_seg_levels(blsbn254_ctx* c, std::vector<uint64_t>& cur, size_t G, std::vector<uint32_t>& start, std::vector<uint32_t>& len,
                    std::vector<SegLevel>& levels, const char* what) {
  const size_t ne = cur.size() - 1;
  std::vector<uint64_t> nxt(ne + 1);
  for (int level = 0; ; ++level) {
    if (level > 40) { c->last_error = what; return BLSBN254_E_HIP; }
    const size_t first = start.size();
    for (size_t e = 0; e < ne; ++e) {
      const uint64_t a = cur[e], b = cur[e + 1];
      nxt[e] = start.size() - first;
      if (a == b) { start.push_back((uint32_t)a); len.push_back(0); }            // empty segment: one empty run (identity, flag 0)
      for (uint64_t s = a; s < b; s += G) { start.push_back((uint32_t)s); len.push_back((uint32_t)std::min<uint64_t>(b - s, G)); }
    }
    const size_t m = start.size() - first;
    nxt[ne] = m;
    levels.push_back({first, m});
    if (m == ne) return 0;
    cur.swap(nxt);
  }
}

// Segmented sums of G2 points: n points already staged at d_pks, groups [goff[g], goff[g + 1]).  Level by level every group is
// cut into chunks of at most G2_SUM_GROUP items, one lane sums a chunk, and the chunk sums (group-major order) are the next
// level's items, until every group is ONE item.  The chunk descriptors of all levels come from the host (the offsets are
// the caller's host array).  On return the sums are at *sum_ws (limb-major, stride = n_groups) with their flags at *sum_ok.
static const size_t G2_SUM_GROUP = 16;
static int g2_group_sums(blsbn254_ctx* c, const uint8_t* d_pks, size_t n, const uint64_t* goff, size_t n_groups, const int32_t** sum_ws, const uint8_t** sum_ok) {
  const size_t G = G2_SUM_GROUP;
  // chunk descriptors of ALL levels first (host arithmetic on the offsets), uploaded in one copy: no synchronisation between levels
  std::vector<uint64_t> cur(goff, goff + n_groups + 1);
  for (size_t g = 0; g <= n_groups; ++g) cur[g] -= goff[0];
  std::vector<uint32_t> start, len;
  std::vector<SegLevel> levels;
  TRY(plan_seg_levels(c, cur, G, start, len, levels, "internal: group sums do not converge"));
  const size_t total = start.size(), m_max = levels[0].count;
  // ping-pong workspaces: the level-0 items (n) and the largest chunk array (the first level's)
  HIPCHK(c, c->gs_ws[0].reserve((n ? n : 1) * 54 * 4)); HIPCHK(c, c->gs_ok[0].reserve(n ? n : 1));
  HIPCHK(c, c->gs_ws[1].reserve(m_max * 54 * 4)); HIPCHK(c, c->gs_ok[1].reserve(m_max));
  HIPCHK(c, c->gs_ws[2].reserve(m_max * 54 * 4)); HIPCHK(c, c->gs_ok[2].reserve(m_max));
  TRY(upload(c, c->gs_start, start.data(), 4 * total));
  TRY(upload(c, c->gs_len, len.data(), 4 * total));
  if (n) TRY(launch(c, c->stream, "g2_load", grid_lanes(n), k_g2_load, d_pks, n, (int32_t*)c->gs_ws[0].p, (uint8_t*)c->gs_ok[0].p));
  int src = 0;
  size_t items = n;
  for (const SegLevel& L : levels) {
    const size_t m = L.count;
    const int dst = src == 1 ? 2 : 1;
    TRY(launch(c, c->stream, "g2_seg_sum", grid_lanes(m), k_g2_seg_sum, (const int32_t*)c->gs_ws[src].p, items ? items : 1, (const uint8_t*)c->gs_ok[src].p,
               (const uint32_t*)c->gs_start.p + L.first, (const uint32_t*)c->gs_len.p + L.first, m, (int32_t*)c->gs_ws[dst].p, m, (uint8_t*)c->gs_ok[dst].p));
    src = dst; items = m;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));                                   // `start` / `len` go out of scope
  *sum_ws = (const int32_t*)c->gs_ws[src].p; *sum_ok = (const uint8_t*)c->gs_ok[src].p;
  return 0;
}

// impl Sum for G2Projective (g2.rs:579-583): out = sum of the n points (the identity encoding for n == 0)
int blsbn254_aggregate_pks(blsbn254_ctx* c, const uint8_t* pks, size_t n, uint8_t out[128]) {
  if (!c || !out || (n && !pks)) return BLSBN254_E_ARG;
  if (n == 0) { std::memset(out, 0, 128); out[127] = 1; return 0; }             // G2Affine::identity: x = 0, y = 1
  if (n > ((size_t)1 << 26)) { c->last_error = "more than 2^26 points in one sum"; return BLSBN254_E_ARG; }
  ENTER(c);
  HIPCHK(c, c->out.reserve(128));
  TRY(upload(c, c->in_a, pks, 128 * n));
  const uint64_t goff[2] = {0, (uint64_t)n};
  const int32_t* ws; const uint8_t* ok;
  int rc = g2_group_sums(c, (const uint8_t*)c->in_a.p, n, goff, 1, &ws, &ok);
  if (rc) return rc;
  uint8_t good = 0;
  TRY(launch(c, c->stream, "g2p_to_bytes", grid_lanes(1), k_g2p_to_bytes, ws, (size_t)1, ok, (size_t)1, (uint8_t*)c->out.p, 0));
  HIPCHK(c, hipMemcpyAsync(out, c->out.p, 128, hipMemcpyDeviceToHost, c->stream));
  TRY(download(c, &good, ok, 1));
  if (!good) { c->last_error = "a point does not decode or is off the curve"; return BLSBN254_ERR_G2; }
  return 0;
}

// FastAggregateVerify per group g: keys pks[key_off[g] .. key_off[g + 1]), ONE message msg_g, ONE signature sig_g:
//   e(sig_g, -G2gen) * e(H(msg_g), sum_k pk_k) == 1
// = CoreVerify under the sum of the group's keys.  The sums are formed on the device (g2_group_sums) and their encodings go
// through the verify pipeline like any public key (KeyValidate on the SUM: not the identity, in the r-torsion).
int blsbn254_fast_aggregate_verify_batch(blsbn254_ctx* c, const uint8_t* pks, const uint64_t* key_off, const uint8_t* msgs, const uint64_t* off,
                                         const uint8_t* sigs, size_t n_groups, const uint8_t* dst, size_t dst_len, uint8_t* valid_bitmap) {
  if (!c || !key_off || !off || (n_groups && (!sigs || !valid_bitmap)) || (dst_len && !dst)) return BLSBN254_E_ARG;
  if (n_groups == 0) return 0;
  for (size_t g = 0; g < n_groups; ++g) if (key_off[g + 1] < key_off[g]) return BLSBN254_E_ARG;
  const size_t n_keys = (size_t)(key_off[n_groups] - key_off[0]);
  if (n_keys && !pks) return BLSBN254_E_ARG;
  if (n_keys > ((size_t)1 << 26) || n_groups > c->chunk) { c->last_error = "more than 2^26 keys or more groups than one launch chunk"; return BLSBN254_E_ARG; }
  ENTER(c);
  uint32_t dl; int rc = stage_dst(c, dst, dst_len, &dl);
  if (rc) return rc;
  rc = stage_msgs(c, msgs, off, n_groups);
  if (rc) return rc;
  const size_t nb = (n_groups + 7) / 8;
  HIPCHK(c, c->in_a.reserve(128 * (n_keys ? n_keys : 1))); HIPCHK(c, c->gs_pk.reserve(128 * n_groups));
  HIPCHK(c, c->bitmap.reserve(nb + 8));
  if (n_keys) HIPCHK(c, hipMemcpyAsync(c->in_a.p, pks + 128 * (size_t)key_off[0], 128 * n_keys, hipMemcpyHostToDevice, c->stream));
  TRY(upload(c, c->in_b, sigs, 64 * n_groups));
  const int32_t* ws; const uint8_t* ok;
  rc = g2_group_sums(c, (const uint8_t*)c->in_a.p, n_keys, key_off, n_groups, &ws, &ok);
  if (rc) return rc;
  TRY(launch(c, c->stream, "g2p_to_bytes", grid_lanes(n_groups), k_g2p_to_bytes, ws, n_groups, ok, n_groups, (uint8_t*)c->gs_pk.p, 1));
  rc = verify_chunk_dev(c, (const uint8_t*)c->gs_pk.p, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, (const uint8_t*)c->in_b.p, n_groups, dl,
                        (uint8_t*)c->bitmap.p);
  if (rc) return rc;
  return download(c, valid_bitmap, c->bitmap.p, nb);
}
int blsbn254_fast_aggregate_verify(blsbn254_ctx* c, const uint8_t* pks, size_t n, const uint8_t* msg, size_t msg_len, const uint8_t sig[64],
                                   const uint8_t* dst, size_t dst_len, int* valid) {
  if (!c || !valid || !sig || (n && !pks) || (msg_len && !msg) || (dst_len && !dst)) return BLSBN254_E_ARG;
  *valid = 0;
  if (n == 0) return 0;
  const uint64_t koff[2] = {0, (uint64_t)n}, moff[2] = {0, (uint64_t)msg_len};
  uint8_t bm = 0;
  int rc = blsbn254_fast_aggregate_verify_batch(c, pks, koff, msg, moff, sig, 1, dst, dst_len, &bm);
  if (rc) return rc;
  *valid = bm & 1;
  return 0;
}

}  // extern "C"
