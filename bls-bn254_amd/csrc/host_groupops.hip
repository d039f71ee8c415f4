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

// Segmented sums of G2 points: n points already staged at d_pks, groups [goff[g], goff[g + 1]).  Level by level every group is
// cut into chunks of at most G2_SUM_GROUP items, one lane sums a chunk, and the chunk sums (group-major order) are the next
// level's items, until every group is ONE item (plan_seg_levels, seg_plan.h; seg_run_levels with k_g2_seg_sum).  The chunk
// descriptors of all levels come from the host (the offsets are the caller's host array) in one copy: nothing synchronises
// between the levels or behind them.  The sums end up in c->gs.sum (limb-major, stride n_groups), their flags in c->gs.sum_ok.
static const size_t G2_SUM_GROUP = 16;
int g2_group_sums(blsbn254_ctx* c, const uint8_t* d_pks, size_t n, const uint64_t* goff, size_t n_groups) {
  SegWs& w = c->gs.seg;
  std::vector<SegRange> seg(n_groups);
  for (size_t g = 0; g < n_groups; ++g) seg[g] = {goff[g] - goff[0], goff[g + 1] - goff[0]};
  w.h_start.clear(); w.h_len.clear();
  std::vector<SegLevel> levels;
  size_t items_max = 1;
  if (!plan_seg_levels(seg, G2_SUM_GROUP, w.h_start, w.h_len, levels, &items_max)) { c->last_error = "internal: group sums do not converge"; return BLSBN254_E_HIP; }
  HIPCHK(c, c->gs.items.reserve((n ? n : 1) * 54 * 4)); HIPCHK(c, c->gs.items_ok.reserve(n ? n : 1));
  HIPCHK(c, c->gs.sum.reserve(n_groups * 54 * 4)); HIPCHK(c, c->gs.sum_ok.reserve(n_groups));
  TRY(seg_stage(c, w, items_max, 54, true));
  if (n) TRY(launch(c, c->stream, "g2_load", grid_lanes(n), k_g2_load, d_pks, n, (int32_t*)c->gs.items.p, (uint8_t*)c->gs.items_ok.p));
  return seg_run_levels(w, levels, {(const int32_t*)c->gs.items.p, n ? n : 1, (const uint8_t*)c->gs.items_ok.p}, {(int32_t*)c->gs.sum.p, n_groups, (uint8_t*)c->gs.sum_ok.p},
                        [&](SegSrc in, const uint32_t* start, const uint32_t* len, size_t runs, SegDst out, bool) {
    return launch(c, c->stream, "g2_seg_sum", grid_lanes(runs), k_g2_seg_sum, in.v, in.stride, in.ok, start, len, runs, out.v, out.stride, out.ok);
  });
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
  TRY(g2_group_sums(c, (const uint8_t*)c->in_a.p, n, goff, 1));
  uint8_t good = 0;
  TRY(launch(c, c->stream, "g2p_to_bytes", grid_lanes(1), k_g2p_to_bytes, (const int32_t*)c->gs.sum.p, (size_t)1, (const uint8_t*)c->gs.sum_ok.p, (size_t)1,
             (uint8_t*)c->out.p, 0));
  HIPCHK(c, hipMemcpyAsync(out, c->out.p, 128, hipMemcpyDeviceToHost, c->stream));
  TRY(download(c, &good, c->gs.sum_ok.p, 1));
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
  HIPCHK(c, c->in_a.reserve(128 * (n_keys ? n_keys : 1))); HIPCHK(c, c->gs.pk.reserve(128 * n_groups));
  HIPCHK(c, c->bitmap.reserve(nb + 8));
  if (n_keys) HIPCHK(c, hipMemcpyAsync(c->in_a.p, pks + 128 * (size_t)key_off[0], 128 * n_keys, hipMemcpyHostToDevice, c->stream));
  TRY(upload(c, c->in_b, sigs, 64 * n_groups));
  TRY(g2_group_sums(c, (const uint8_t*)c->in_a.p, n_keys, key_off, n_groups));
  TRY(launch(c, c->stream, "g2p_to_bytes", grid_lanes(n_groups), k_g2p_to_bytes, (const int32_t*)c->gs.sum.p, n_groups, (const uint8_t*)c->gs.sum_ok.p, n_groups,
             (uint8_t*)c->gs.pk.p, 1));
  rc = verify_chunk_dev(c, (const uint8_t*)c->gs.pk.p, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, (const uint8_t*)c->in_b.p, n_groups, dl,
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
