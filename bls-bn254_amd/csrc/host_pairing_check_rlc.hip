// host_pairing_check_rlc.hip -- pairing-product equations over ragged groups of pairs by random linear combination across equations:
// the bitmap of blsbn254_pairing_check_batch (multi_miller_loop(..).final_exponentiation() == Gt::identity, pairings.rs:706-713
// with :698-704) from u table-only Miller loops and one final exponentiation where the G2 members repeat.  Host side of
// include/blsbn254.h; kernels in k_pairing_check_rlc.hip, lane functions in pairing_check_rlc.h, the plan in
// pairing_check_rlc_plan.h over aggregate_rlc_plan.h; see host_common.h and DESIGN.md 6w.
//
// A call: the G2 members de-duplicated by their bytes (dedup_keys: u distinct; members that do not repeat: the exact call, nothing
// else), their raw line tables on the second stream (raw_tables_fork: the key preparation tests each DISTINCT Q once), then
// k_pcr_pairs, k_pcr_eq and k_pcr_weigh leave r_g P_gj in ONE workspace that stays on the device for both rounds.  A round is
// agr_round without signature slots (host_aggregate_rlc.hip): virtual key id segment * u + key id, the sums per virtual key, the
// S u sums paired with their Q's tables, the segments' products, ONE run_final_exp.  Whatever the rounds do not decide goes to
// blsbn254_pairing_check_batch on contiguous equation ranges: a pointer offset, not a repack.  Nothing a round or the bits need
// after a sub-call lives in what the exact call overwrites (in_a, in_b, f_ws, pc.*): the sub-calls run last.
#include "host_common.h"

extern "C" {

// the call IS the exact call: counted, every equation as sent to the exact pipeline
static int pcr_exact(blsbn254_ctx* c, const uint8_t* g1, const uint8_t* g2, const uint64_t* off, size_t G, uint8_t* valid_bitmap) {
  TRY(blsbn254_pairing_check_batch(c, g1, g2, off, G, valid_bitmap));
  ++c->pcr.stat[0]; ++c->pcr.stat[6]; c->pcr.stat[3] += G;
  return 0;
}

int blsbn254_pairing_check_batch_rlc(blsbn254_ctx* c, const uint8_t* g1, const uint8_t* g2, const uint64_t* off, size_t n_eq, const uint8_t seed[32],
                                     uint8_t* valid_bitmap) {
  if (!c) return BLSBN254_E_ARG;
  if (n_eq == 0) return 0;
  TRY(pc_args(c, g1, g2, off, n_eq, valid_bitmap));
  const size_t G = n_eq, base = (size_t)off[0], N = (size_t)(off[G] - off[0]);
  Stream2Guard s2_guard(c);
  ENTER(c);
  if (N == 0) return pcr_exact(c, g1, g2, off, G, valid_bitmap);      // every equation is empty and holds: nothing to combine
  PcrWs& w = c->pcr;
  // Q into in_a (where the key preparation reads its keys), P into in_b
  TRY(upload(c, c->in_a, g2 + 128 * base, 128 * N));
  TRY(upload(c, c->in_b, g1 + 64 * base, 64 * N));
  size_t u = 0;
  TRY(dedup_keys(c, (const uint8_t*)c->in_a.p, N, &u));
  if (!pcr_round1(N, u, PREP_MAX_KEYS)) return pcr_exact(c, g1, g2, off, G, valid_bitmap);
  TRY(raw_tables_fork(c, u));                           // the u distinct Q: line tables and validity bytes, beside what follows
  TRY(stage_seed(c, w.seed, seed));
  // the plan: the segments of a second round are known before the first, so the workspace is reserved once
  size_t S2 = agr_segments(c->pcr_segments, PCR_SMAX, N, u, G);
  if (S2 * u > MAX_LANES) S2 = 1;                       // the slots of a round are one launch's stride
  const size_t W = N + S2 * u, nb = (G + 7) / 8;
  agr_pair_groups(off, G, w.h_gidx);
  TRY(upload(c, w.gidx, w.h_gidx.data(), 4 * N));
  TRY(stage_group_offsets(c, w.goff, off, G));
  HIPCHK(c, w.pts.reserve(N * 18 * 4)); HIPCHK(c, w.flag.reserve(N)); HIPCHK(c, w.w.reserve(W * 27 * 4)); HIPCHK(c, w.vkid.reserve(4 * W));
  HIPCHK(c, w.elig.reserve(G)); HIPCHK(c, w.wt.reserve(8 * G));
  TRY(dedup_key_ids(c, N, u, false));
  HIPCHK(c, join_stream2(c));                           // the validity bytes of the distinct Q are final
  TRY(launch(c, c->stream, "pcr_pairs", grid_lanes(N), k_pcr_pairs, (const uint8_t*)c->in_b.p, (const uint8_t*)c->in_a.p, (const uint32_t*)c->kd.kid.p, (const uint8_t*)c->prep.ok.p, N,
             (int32_t*)w.pts.p, (uint8_t*)w.flag.p));
  TRY(launch(c, c->stream, "pcr_eq", grid_lanes(G), k_pcr_eq, (const uint32_t*)w.goff.d.p, (const uint8_t*)w.flag.p, (const uint8_t*)w.seed.p, G, (uint8_t*)w.elig.p, (uint2*)w.wt.p));
  TRY(launch(c, c->stream, "pcr_weigh", grid_lanes((N + 1) / 2), k_pcr_weigh, (const int32_t*)w.pts.p, N, (const uint32_t*)w.gidx.p, (const uint8_t*)w.flag.p, (const uint8_t*)w.elig.p,
             (const uint2*)w.wt.p, (int32_t*)w.w.p, W));
  w.h_elig.resize(G);
  HIPCHK(c, hipMemcpyAsync(w.h_elig.data(), w.elig.p, G, hipMemcpyDeviceToHost, c->stream));
  // round 1: all eligible equations as ONE combined equation
  TRY(agr_round(c, w, N, G, u, 1, W, nullptr, false));
  size_t n_elig = 0;
  for (size_t g = 0; g < G; ++g) n_elig += w.h_elig[g] ? 1 : 0;
  uint64_t equations = 1, by_round2 = 0, failed_segments = 0;
  size_t n_exact = 0;
  const bool pass1 = w.h_pass[0] != 0;
  if (pass1) {
    TRY(agr_bits(c, w, G, nullptr, valid_bitmap));
  } else {
    // round 2: S2 segments of consecutive equations in one batched pass over the same weighted points
    if (S2 >= 2) {
      agr_cut(G, S2, w.h_bound, w.h_seg_of);
      TRY(upload(c, w.seg_of, w.h_seg_of.data(), 4 * G));
      TRY(agr_round(c, w, N, G, u, S2, W, (const uint32_t*)w.seg_of.p, false));
      TRY(agr_bits(c, w, G, (const uint32_t*)w.seg_of.p, valid_bitmap));
      equations += S2;
      for (size_t s = 0; s < S2; ++s) failed_segments += w.h_pass[s] ? 0 : 1;
      for (size_t g = 0; g < G; ++g) by_round2 += (w.h_elig[g] && w.h_pass[w.h_seg_of[g]]) ? 1 : 0;
    } else {
      w.h_bound.assign({0u, (uint32_t)G});
      std::memset(valid_bitmap, 0, nb);
    }
    // the exact call decides the eligible equations of the failed segments, on their contiguous ranges (close ranges as one);
    // off need not start at 0, so a range is a pointer offset into the caller's offsets
    agr_failed_ranges(w.h_bound, w.h_pass.data(), w.h_elig.data(), off, PCR_MERGE_GAP, w.ranges, &n_exact);
    for (const std::pair<size_t, size_t>& r : w.ranges) {
      const size_t a = r.first, m = r.second - r.first;
      w.h_bits.assign((m + 7) / 8, 0);
      TRY(blsbn254_pairing_check_batch(c, g1, g2, off + a, m, w.h_bits.data()));
      for (size_t j = 0; j < m; ++j)
        if (w.h_elig[a + j] && bit_at(w.h_bits.data(), j)) set_bit(valid_bitmap, a + j);
    }
  }
  ++w.stat[0]; w.stat[1] += pass1 ? n_elig : 0; w.stat[2] += by_round2; w.stat[3] += n_exact;
  w.stat[4] += G - n_elig; w.stat[5] += equations; w.stat[7] += failed_segments;      // counted once the call has succeeded
  return 0;
}

int blsbn254_set_pairing_check_rlc_segments(blsbn254_ctx* c, size_t segments) {
  if (!c || segments > AGR_MAX_SEGMENTS) return BLSBN254_E_ARG;
  c->pcr_segments = segments;
  return 0;
}
int blsbn254_pairing_check_rlc_stats(blsbn254_ctx* c, uint64_t out[8]) { return COPY_STATS(c, pcr.stat, 8, out); }

}  // extern "C"
