// host_aggregate_rlc.hip -- aggregate verify over ragged groups of (key, message) pairs by random linear combination across groups:
// the bitmap of blsbn254_aggregate_verify_batch from u + 1 table-only Miller loops and one final exponentiation where the keys
// repeat.  Host side of include/blsbn254.h; kernels in k_aggregate_rlc.hip, lane functions in aggregate_rlc.h, the plan in
// aggregate_rlc_plan.h; see host_common.h and DESIGN.md 6s.
//
// A call: the keys de-duplicated (agg_keys_stage: u distinct keys; keys that do not repeat: the exact call, nothing else), their raw
// line tables and -G2gen's (table u) on the second stream beside the hashing (agg_keys_prepare), the hash points homogeneous
// (k_hash_to_g1 mode 3), then k_agr_group and k_agr_weigh leave r_g sig_g and r_g H_gi in ONE workspace that stays on the device
// for both rounds.  A round over S segments (agr_round; S = 1: the whole call) gives every item the virtual key id
// segment * u + key id (a signature: S u + segment), sums the items per virtual key (key_sorted_order, key_sums), and pairs the
// S (u + 1) sums with their keys' tables in the form that fits the launch (launch_miller_raw, host_aggregate.hip); the segments'
// products (fp12_tree; k_fp12_seg_prod by levels and the signatures' values multiplied in) finish in ONE run_final_exp.  Whatever
// the rounds do not decide goes to blsbn254_aggregate_verify_batch on contiguous group ranges: a pointer offset, not a repack.
#include "host_common.h"

extern "C" {

// One round: the is-one byte of every segment into w.h_pass (synchronised).  d_seg_of: the groups' segments on the device,
// nullptr for S == 1.  W: the stride of the workspace w.w, whose columns behind the items (N + G .. N + G + S (u + 1); without
// signature slots N .. N + S u) this round pads.  The pairing-product checks (host_pairing_check_rlc.hip) run the same round
// without signature slots: their items kernel, no signature value multiplied in, everything else launch for launch.
int agr_round(blsbn254_ctx* c, AgrWs& w, size_t N, size_t G, size_t u, size_t S, size_t W, const uint32_t* d_seg_of, bool sig_slots) {
  if (!sig_slots) G = 0;
  const size_t V = S * (u + (sig_slots ? 1 : 0)), items = N + G + V;
  const uint32_t u32 = (uint32_t)u, S32 = (uint32_t)S;
  uint32_t* vkid = (uint32_t*)w.vkid.p;
  HIPCHK(c, w.mkid.reserve(4 * V));
  if (sig_slots)
    TRY(launch(c, c->stream, "agr_items", grid_lanes(items), k_agr_items, (const uint32_t*)w.gidx.p, (const uint32_t*)c->kd.kid.p, d_seg_of, N, G, u32, S32, (int32_t*)w.w.p, W,
               vkid, (uint32_t*)w.mkid.p));
  else
    TRY(launch(c, c->stream, "pcr_items", grid_lanes(items), k_pcr_items, (const uint32_t*)w.gidx.p, (const uint32_t*)c->kd.kid.p, d_seg_of, N, u32, S32, (int32_t*)w.w.p, W,
               vkid, (uint32_t*)w.mkid.p));
  // the items' histogram over the virtual keys (every id is below V by construction: the check cannot fail), the sorted order, the sums
  HIPCHK(c, c->kd.hist.reserve(4 * (V + 2)));
  TRY(check_key_indices(c, vkid, items, V, (uint32_t*)c->kd.hist.p, "pair", false));
  TRY(key_sorted_order(c, vkid, items, V));
  const uint32_t *hist = (const uint32_t*)c->kd.hist.p, *cursor = (const uint32_t*)c->kd.cursor.p, *perm = (const uint32_t*)c->kd.perm.p;
  const int32_t* pts = nullptr;
  TRY(key_sums(c, (const int32_t*)w.w.p, nullptr, W, perm, perm, vkid, hist, cursor, items, V, &pts, nullptr));
  // the V pairs (sum, its key's table); a sum that is the identity contributes 1 (status bit 1: the loops' skip)
  HIPCHK(c, w.h2.reserve(V * 18 * 4)); HIPCHK(c, w.st.reserve(V)); HIPCHK(c, w.isone.reserve(S));
  TRY(launch(c, c->stream, "g1p_to_h", grid_lanes(V), k_g1p_to_h_affine, pts, V, V, (int32_t*)w.h2.p, V, (uint8_t*)w.st.p));
  // S > 1: never two slots per lane, because a lane's value must belong to ONE segment slot
  size_t f_cnt;
  TRY(launch_miller_raw(c, (const int32_t*)w.h2.p, V, (const uint32_t*)w.mkid.p, {(const int32_t*)c->prep.raw.p, (const uint8_t*)c->prep.ok.p}, V, (const uint8_t*)w.st.p,
                        S == 1 ? MR_ALL : MR_ALL & ~MR_TWO, &f_cnt));
  int32_t* f = (int32_t*)c->f_ws.p;
  // (the loops' flags are not read: a key that is not valid belongs to ineligible groups only, so its sums are the identity)
  int32_t* prod; size_t ps;
  if (S == 1) {
    TRY(fp12_tree(c, f, f_cnt, f_cnt, &prod, &ps));
  } else {
    // segment s: the product of its u key slots s u .. (s + 1) u by levels, then its signature slot S u + s multiplied in
    std::vector<SegRange> seg(S);
    for (size_t s = 0; s < S; ++s) seg[s] = {s * u, (s + 1) * u};
    std::vector<SegLevel> levels;
    size_t items_max = 1;
    w.seg.h_start.clear(); w.seg.h_len.clear();
    if (!plan_seg_levels(seg, FP12_SEG_GROUP, w.seg.h_start, w.seg.h_len, levels, &items_max)) {
      c->last_error = "internal: segmented products do not converge";
      return BLSBN254_E_HIP;
    }
    HIPCHK(c, w.prod.reserve(S * 108 * 4));
    TRY(seg_stage(c, w.seg, items_max, 108, false));
    prod = (int32_t*)w.prod.p; ps = S;
    TRY(seg_run_levels(w.seg, levels, {(const int32_t*)f, V, nullptr}, {prod, S, nullptr},
                       [&](SegSrc in, const uint32_t* start, const uint32_t* len, size_t runs, SegDst out, bool) {
      return launch(c, c->stream, "fp12_seg_prod", grid_lanes(runs), k_fp12_seg_prod, in.v, in.stride, in.ok, start, len, runs, out.v, out.stride, out.ok, 0);
    }));
    if (sig_slots) TRY(launch(c, c->stream, "fp12_mul_elem", grid_lanes(S), k_fp12_mul_elem, prod, S, (const int32_t*)f + S * u, V, S));
  }
  TRY(run_final_exp(c, prod, S, ps, 4, nullptr, nullptr, nullptr, (uint8_t*)w.isone.p, nullptr));
  w.h_pass.resize(S);
  return download(c, w.h_pass.data(), w.isone.p, S);
}

// valid = eligible and the segment's equation held, packed into c->bitmap and downloaded
int agr_bits(blsbn254_ctx* c, AgrWs& w, size_t G, const uint32_t* d_seg_of, uint8_t* bm) {
  HIPCHK(c, w.valid.reserve(G)); HIPCHK(c, c->bitmap.reserve((G + 7) / 8 + 8));
  TRY(launch(c, c->stream, "agr_bits", grid_lanes(G), k_agr_bits, (const uint8_t*)w.elig.p, d_seg_of, (const uint8_t*)w.isone.p, G, (uint8_t*)w.valid.p));
  TRY(launch(c, c->stream, "pack_bitmap", grid_lanes(G), k_pack_bitmap, (const uint8_t*)w.valid.p, G, (uint8_t*)c->bitmap.p));
  return download(c, bm, c->bitmap.p, (G + 7) / 8);
}

// The call behind its entry points.  want_dup (blsbn254_aggregate_verify_batch_rlc_distinct): the distinct-message stage runs on
// the homogeneous hash points behind the hashing launch -- once, for all groups, so the exact sub-calls of failed ranges run
// without it -- and leaves the groups' repeat bits in c->md.h_bits; a call whose keys do not repeat hands the request to the exact call.
// Without it the launch sequence, the results and the counters are what they were before the stage existed.
int aggregate_verify_batch_rlc_impl(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, const uint64_t* grp_off,
                                    const uint8_t* agg_sigs, size_t n_groups, const uint8_t* dst, size_t dst_len, const uint8_t* seed,
                                    uint8_t* valid_bitmap, bool want_dup, const char* call) {
  const int args = agg_batch_args(c, pks, msgs, off, grp_off, agg_sigs, n_groups, dst, dst_len, valid_bitmap, call);
  if (args) return args == CK_NOTHING ? 0 : args;
  const size_t G = n_groups, base = (size_t)grp_off[0], N = (size_t)(grp_off[G] - grp_off[0]);
  Stream2Guard s2_guard(c);
  ENTER(c);                                             // settles pending asynchronous verify calls BEFORE the tag is staged
  const size_t nb = (G + 7) / 8;
  if (N == 0) {                                         // every group is empty: invalid, nothing to launch
    std::memset(valid_bitmap, 0, nb);
    ++c->agr.stat[0]; c->agr.stat[4] += G;
    if (want_dup) { c->md.h_bits.assign(nb, 0); ++c->md.stat[0]; c->md.stat[3] = 0; }      // ... and none is repeated
    return 0;
  }
  uint32_t dl = 0;
  TRY(stage_dst(c, dst, dst_len, &dl));
  TRY(stage_msgs(c, msgs, off + base, N));
  AgrWs& w = c->agr;
  size_t u = 0;
  TRY(agg_keys_stage(c, pks + 128 * base, N, &u));     // the keys with -G2gen as "pair N" (the key of the signatures' slots), de-duplicated
  if (!agr_keys_repeat(N, u, PREP_MAX_KEYS)) {          // nothing to share per key: the call is the exact call
    TRY(aggregate_verify_batch_impl(c, pks, msgs, off, grp_off, agg_sigs, G, dst, dst_len, valid_bitmap, want_dup, call));
    ++c->agr.stat[0]; ++c->agr.stat[6]; c->agr.stat[3] += G;
    return 0;
  }
  TRY(stage_seed(c, w.seed, seed));
  TRY(upload(c, c->in_b, agg_sigs, 64 * G));
  TRY(agg_keys_prepare(c, N, u));                      // the u keys and -G2gen (key id u): line tables beside the hashing
  // the plan: the segments of a second round are known before the first, so the workspace is reserved once
  size_t S2 = agr_segments(c->agr_segments, AGR_SMAX, N, u, G);
  if (S2 * (u + 1) > MAX_LANES) S2 = 1;                 // the slots of a round are one launch's stride
  const size_t W = N + G + S2 * (u + 1);
  agr_pair_groups(grp_off, G, w.h_gidx);
  TRY(upload(c, w.gidx, w.h_gidx.data(), 4 * N));
  TRY(stage_group_offsets(c, w.goff, grp_off, G));
  HIPCHK(c, c->h_ws.reserve(N * 27 * 4)); HIPCHK(c, w.w.reserve(W * 27 * 4)); HIPCHK(c, w.vkid.reserve(4 * W));
  HIPCHK(c, w.sig_ok.reserve(G)); HIPCHK(c, w.elig.reserve(G)); HIPCHK(c, w.wt.reserve(8 * G));
  TRY(dedup_key_ids(c, N, u, false));
  TRY(launch_hash_to_g1(c, c->stream, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, N, dl, (int32_t*)c->h_ws.p, N,
             (uint8_t*)nullptr, 3));
  if (want_dup) TRY(msg_distinct_stage(c, (const int32_t*)c->h_ws.p, N, N, MD_HOMOGENEOUS, (const uint32_t*)w.goff.d.p, G));
  HIPCHK(c, join_stream2(c));                           // the keys' validity bytes are final
  TRY(launch(c, c->stream, "agr_group", grid_lanes(G), k_agr_group, (const uint8_t*)c->in_b.p, (const uint32_t*)w.goff.d.p, (const uint32_t*)c->kd.kid.p, (const uint8_t*)c->prep.ok.p, (const uint8_t*)w.seed.p, G,
             (uint8_t*)w.sig_ok.p, (uint8_t*)w.elig.p, (uint2*)w.wt.p, (int32_t*)w.w.p, W, N));
  TRY(launch(c, c->stream, "agr_weigh", grid_lanes((N + 1) / 2), k_agr_weigh, (const int32_t*)c->h_ws.p, N, (const uint32_t*)w.gidx.p, (const uint8_t*)w.elig.p,
             (const uint2*)w.wt.p, (int32_t*)w.w.p, W));
  w.h_elig.resize(G);
  HIPCHK(c, hipMemcpyAsync(w.h_elig.data(), w.elig.p, G, hipMemcpyDeviceToHost, c->stream));
  // round 1: all eligible groups as ONE virtual aggregate
  TRY(agr_round(c, w, N, G, u, 1, W, nullptr, true));
  size_t n_elig = 0;
  for (size_t g = 0; g < G; ++g) n_elig += w.h_elig[g] ? 1 : 0;
  uint64_t equations = 1, by_round2 = 0, failed_segments = 0;
  size_t n_exact = 0;
  const bool pass1 = w.h_pass[0] != 0;
  if (pass1) {
    TRY(agr_bits(c, w, G, nullptr, valid_bitmap));
  } else {
    // round 2: S2 segments of consecutive groups in one batched pass over the same weighted points
    if (S2 >= 2) {
      agr_cut(G, S2, w.h_bound, w.h_seg_of);
      TRY(upload(c, w.seg_of, w.h_seg_of.data(), 4 * G));
      TRY(agr_round(c, w, N, G, u, S2, W, (const uint32_t*)w.seg_of.p, true));
      TRY(agr_bits(c, w, G, (const uint32_t*)w.seg_of.p, valid_bitmap));
      equations += S2;
      for (size_t s = 0; s < S2; ++s) failed_segments += w.h_pass[s] ? 0 : 1;
      for (size_t g = 0; g < G; ++g) by_round2 += (w.h_elig[g] && w.h_pass[w.h_seg_of[g]]) ? 1 : 0;
    } else {
      w.h_bound.assign({0u, (uint32_t)G});
      std::memset(valid_bitmap, 0, nb);
    }
    // the exact pipeline decides the eligible groups of the failed segments, on their contiguous ranges (close ranges as one)
    agr_failed_ranges(w.h_bound, w.h_pass.data(), w.h_elig.data(), grp_off, AGR_MERGE_GAP, w.ranges, &n_exact);
    for (const std::pair<size_t, size_t>& r : w.ranges) {
      const size_t a = r.first, m = r.second - r.first;
      w.h_bits.assign((m + 7) / 8, 0);
      TRY(blsbn254_aggregate_verify_batch(c, pks, msgs, off, grp_off + a, agg_sigs + 64 * a, m, dst, dst_len, w.h_bits.data()));
      for (size_t j = 0; j < m; ++j)
        if (w.h_elig[a + j] && bit_at(w.h_bits.data(), j)) set_bit(valid_bitmap, a + j);
    }
  }
  if (want_dup) TRY(msg_distinct_bits(c, N, G, nullptr));
  ++c->agr.stat[0]; c->agr.stat[1] += pass1 ? n_elig : 0; c->agr.stat[2] += by_round2; c->agr.stat[3] += n_exact;
  c->agr.stat[4] += G - n_elig; c->agr.stat[5] += equations; c->agr.stat[7] += failed_segments;      // counted once the call has succeeded
  return 0;
}
int blsbn254_aggregate_verify_batch_rlc(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, const uint64_t* grp_off,
                                        const uint8_t* agg_sigs, size_t n_groups, const uint8_t* dst, size_t dst_len, const uint8_t seed[32],
                                        uint8_t* valid_bitmap) {
  return aggregate_verify_batch_rlc_impl(c, pks, msgs, off, grp_off, agg_sigs, n_groups, dst, dst_len, seed, valid_bitmap, false, "aggregate_verify_batch_rlc");
}

int blsbn254_set_aggregate_rlc_segments(blsbn254_ctx* c, size_t segments) {
  if (!c || segments > AGR_MAX_SEGMENTS) return BLSBN254_E_ARG;
  c->agr_segments = segments;
  return 0;
}
int blsbn254_aggregate_rlc_stats(blsbn254_ctx* c, uint64_t out[8]) { return COPY_STATS(c, agr.stat, 8, out); }

}  // extern "C"
