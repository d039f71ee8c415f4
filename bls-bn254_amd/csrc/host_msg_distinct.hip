// host_msg_distinct.hip -- the distinct-message rule of the aggregate verify over groups: group g is REPEATED when two of its
// pairs have the same hash point.  Host side of include/blsbn254.h; kernels in k_msg_distinct.hip, lane functions in
// msg_distinct.h; see host_common.h and DESIGN.md 6v.
//
// ONE stage, msg_distinct_stage, over hash points that are on the device already: the exact pipeline's affine workspace
// (host_aggregate_batch.hip, mode 0) or the RLC pipeline's homogeneous one (host_aggregate_rlc.hip, mode 3), so the two verify
// calls hash nothing twice and download no point; blsbn254_hash_distinct_batch hashes as blsbn254_hash_to_g1_batch does and runs
// nothing else.  Per pair the stage holds 72 bytes of canonical (x, y), 8 .. 16 bytes of slot table and, per group, one byte.
#include "host_common.h"

extern "C" {

int msg_distinct_stage(blsbn254_ctx* c, const int32_t* pts, size_t stride, size_t N, int form, const uint32_t* d_goff, size_t G) {
  MdWs& w = c->md;
  if (N > MAX_LANES || G > MAX_LANES) { c->last_error = "internal: the distinct-message stage spans more than 2^23 pairs"; return BLSBN254_E_HIP; }
  const uint32_t M = md_slots((uint32_t)N);
  HIPCHK(c, w.dup.reserve(G)); HIPCHK(c, w.slots.reserve(4 * (size_t)M)); HIPCHK(c, w.key.reserve(4 * (size_t)MD_KEY_LIMBS * N));
  HIPCHK(c, hipMemsetAsync(w.dup.p, 0, G, c->stream));                           // every call starts from a cleared table
  HIPCHK(c, hipMemsetAsync(w.slots.p, 0xff, 4 * (size_t)M, c->stream));          // ... KC_EMPTY in every slot
  if (N == 0) return 0;
  TRY(launch(c, c->stream, "md_keys", grid_lanes(N), k_md_keys, pts, stride, (uint32_t)N, form, (int32_t*)w.key.p));
  TRY(launch(c, c->stream, "md_insert", grid_lanes(N), k_md_insert, (uint32_t)N, d_goff, (uint32_t)G, (const int32_t*)w.key.p, (uint32_t*)w.slots.p, M - 1, c->kd.seed,
             (uint8_t*)w.dup.p));
  return 0;
}

int msg_distinct_bits(blsbn254_ctx* c, size_t N, size_t G, uint8_t* dup_bitmap) {
  MdWs& w = c->md;
  const size_t nb = (G + 7) / 8;
  HIPCHK(c, w.bits.reserve(nb + 8));
  TRY(launch(c, c->stream, "pack_bitmap", grid_lanes(G), k_pack_bitmap, (const uint8_t*)w.dup.p, G, (uint8_t*)w.bits.p));
  w.h_bits.assign(nb, 0);
  TRY(download(c, w.h_bits.data(), w.bits.p, nb));
  if (G & 7) w.h_bits[nb - 1] &= (uint8_t)((1u << (G & 7)) - 1);
  uint64_t repeated = 0;
  for (size_t j = 0; j < nb; ++j) repeated += (uint64_t)__builtin_popcount(w.h_bits[j]);
  if (dup_bitmap) std::memcpy(dup_bitmap, w.h_bits.data(), nb);
  ++w.stat[0]; w.stat[1] += N; w.stat[2] += repeated; w.stat[3] = md_slots((uint32_t)N);      // counted once the call has succeeded
  return 0;
}

int blsbn254_hash_distinct_batch(blsbn254_ctx* c, const uint8_t* msgs, const uint64_t* off, const uint64_t* grp_off, size_t n_groups, const uint8_t* dst,
                                 size_t dst_len, uint8_t* dup_bitmap) {
  const int args = agg_msg_args(c, msgs, off, grp_off, n_groups, dst, dst_len, !dup_bitmap, false, "hash_distinct_batch");      // the rules of agg_batch_args
  if (args) return args == CK_NOTHING ? 0 : args;
  const size_t G = n_groups, base = (size_t)grp_off[0], N = (size_t)(grp_off[G] - grp_off[0]);
  ENTER(c);
  if (N == 0) {                                         // every group is empty: none is repeated, nothing to launch
    std::memset(dup_bitmap, 0, (G + 7) / 8);
    ++c->md.stat[0]; c->md.stat[3] = 0;
    return 0;
  }
  uint32_t dl = 0;
  TRY(stage_dst(c, dst, dst_len, &dl));
  TRY(stage_msgs(c, msgs, off + base, N));
  TRY(stage_group_offsets(c, c->md.goff, grp_off, G));
  HIPCHK(c, c->h_ws.reserve(N * 18 * 4));
  TRY(launch_hash_to_g1(c, c->stream, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, N, dl, (int32_t*)c->h_ws.p, N, (uint8_t*)nullptr, 0));
  TRY(msg_distinct_stage(c, (const int32_t*)c->h_ws.p, N, N, MD_AFFINE, (const uint32_t*)c->md.goff.d.p, G));
  return msg_distinct_bits(c, N, G, dup_bitmap);
}

// valid &= ~dup over the two host bitmaps of a call whose stage left its bits in c->md.h_bits
static void clear_repeated(const blsbn254_ctx* c, size_t G, uint8_t* valid_bitmap) {
  for (size_t j = 0; j < (G + 7) / 8; ++j) valid_bitmap[j] &= (uint8_t)~c->md.h_bits[j];
}

int blsbn254_aggregate_verify_batch_distinct(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, const uint64_t* grp_off,
                                             const uint8_t* agg_sigs, size_t n_groups, const uint8_t* dst, size_t dst_len, uint8_t* valid_bitmap,
                                             uint8_t* dup_bitmap) {
  TRY(aggregate_verify_batch_impl(c, pks, msgs, off, grp_off, agg_sigs, n_groups, dst, dst_len, valid_bitmap, true, "aggregate_verify_batch_distinct"));
  if (n_groups == 0) return 0;
  clear_repeated(c, n_groups, valid_bitmap);
  if (dup_bitmap) std::memcpy(dup_bitmap, c->md.h_bits.data(), (n_groups + 7) / 8);
  return 0;
}
int blsbn254_aggregate_verify_batch_rlc_distinct(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, const uint64_t* grp_off,
                                                 const uint8_t* agg_sigs, size_t n_groups, const uint8_t* dst, size_t dst_len, const uint8_t seed[32],
                                                 uint8_t* valid_bitmap, uint8_t* dup_bitmap) {
  TRY(aggregate_verify_batch_rlc_impl(c, pks, msgs, off, grp_off, agg_sigs, n_groups, dst, dst_len, seed, valid_bitmap, true,
                                      "aggregate_verify_batch_rlc_distinct"));
  if (n_groups == 0) return 0;
  clear_repeated(c, n_groups, valid_bitmap);
  if (dup_bitmap) std::memcpy(dup_bitmap, c->md.h_bits.data(), (n_groups + 7) / 8);
  return 0;
}

int blsbn254_msg_distinct_stats(blsbn254_ctx* c, uint64_t out[4]) { return COPY_STATS(c, md.stat, 4, out); }

}  // extern "C"
