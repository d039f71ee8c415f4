// host_threshold_batch.hip -- threshold combine and Lagrange coefficients over ragged groups of shares: n_groups independent
// blsbn254_threshold_combine / blsbn254_lagrange_at_zero in one call.  Host side of include/blsbn254.h; kernels in
// k_threshold_batch.hip (one lane per SHARE over all groups of a launch); see host_common.h.
//
// All ids and partial signatures are uploaded once.  The shares run in launches of at most ctx->chunk shares that end on a
// group boundary (a launch always takes at least one whole group): ids decoded, Lagrange coefficients per lane over the lane's
// group, [lambda] sigma per lane, then each group's products summed level by level (seg_run_levels with k_g1_seg_sum; the last
// level writes into the per-group sums, limb-major, stride n_groups).  After the last launch: one inversion per group
// (k_g1p_to_bytes), the per-group marks folded into statuses (k_th_finish), ONE download and synchronisation.  All launches and
// their levels are planned on the host up front (plan_launches_whole, seg_plan.h) and the descriptors uploaded in one copy.
//
// Groups of more than TH_BATCH_TBIG shares do not take that path: the per-lane Lagrange loop is quadratic in the group and serial in
// the lane, which the single-group pipeline (t x sqrt(t) lanes, host_aggregate.hip) avoids.  Their lanes only test their point
// here (decodes, on the curve -- the single pipeline tests only the decoding; such a group may be cut by a launch boundary
// anywhere, its lanes are independent), their sum slot gets the identity, and after the synchronisation each goes through
// threshold_combine_one / lagrange_one into its slot of the caller's outputs.
#include "host_common.h"

// The hand-over size.  In the sweep that places it (16 equal groups per call, t = 64 .. 4096, profiles/threshold_batch.json,
// DESIGN.md 6d) the loop of single calls never became faster than the lane-per-share kernels, so it sits at the end of the
// sweep.  A compile-time constant on purpose (not an option, not an environment variable); -DBN_TH_BATCH_TBIG=<n> is for the
// measurement build of that sweep (scripts/bench_threshold_batch.py).
#ifndef BN_TH_BATCH_TBIG
#define BN_TH_BATCH_TBIG 4096
#endif

extern "C" {

static const size_t TH_BATCH_TBIG = BN_TH_BATCH_TBIG;
static const size_t TH_SUM_GROUP = 16;      // products per lane and level of the group sums

size_t th_batch_tbig() { return TH_BATCH_TBIG; }

// The device part for all groups, on ids (and partial signatures) already on the device: per-group statuses into c->thb.st, and
// with `d_sigs` the encodings into c->thb.out, else the coefficients into c->scalars.  Everything is enqueued; the caller
// downloads and synchronises.
int th_enqueue_dev(blsbn254_ctx* c, const uint8_t* d_ids, const uint8_t* d_sigs, const uint64_t* off, size_t n_groups) {
  const bool sigs = d_sigs != nullptr;
  ThbWs& w = c->thb;
  TRY(stage_group_offsets(c, w.goff, off, n_groups));
  const size_t N = w.goff.h[n_groups];
  w.seg.h_start.clear(); w.seg.h_len.clear();
  std::vector<SegLaunch> launches;
  size_t m_max, items_max;
  if (!plan_launches_whole(w.goff.h, n_groups, c->chunk, TH_SUM_GROUP, TH_BATCH_TBIG, launches, w.seg.h_start, w.seg.h_len, &m_max, &items_max)) {
    c->last_error = "internal: group sums do not converge";
    return BLSBN254_E_HIP;
  }
  const size_t m1 = m_max ? m_max : 1, N1 = N ? N : 1;
  HIPCHK(c, c->th.x.reserve(9 * m1 * 4)); HIPCHK(c, c->th.glv.reserve(9 * m1 * 4)); HIPCHK(c, c->status.reserve(m1));
  HIPCHK(c, w.gid.reserve(4 * m1)); HIPCHK(c, w.gstat.reserve(4 * n_groups)); HIPCHK(c, w.st.reserve(n_groups));
  if (sigs) {
    HIPCHK(c, w.pts.reserve(27 * m1 * 4)); HIPCHK(c, w.gsum.reserve(27 * n_groups * 4)); HIPCHK(c, w.out.reserve(64 * n_groups));
    TRY(seg_stage(c, w.seg, items_max, 27, false));
  } else HIPCHK(c, c->scalars.reserve(32 * N1));
  HIPCHK(c, hipMemsetAsync(w.gstat.p, 0, 4 * n_groups, c->stream));
  const uint32_t* goff = (const uint32_t*)w.goff.d.p;
  uint32_t* gstat = (uint32_t*)w.gstat.p;
  for (const SegLaunch& L : launches) {
    const size_t m = L.hi - L.lo;
    ++c->thb.stat[2];
    if (m) {
      TRY(launch(c, c->stream, "fr_decode", grid_lanes(m), k_fr_decode, d_ids + 32 * L.lo, m, (int32_t*)c->th.x.p, (uint8_t*)c->status.p));
      TRY(launch(c, c->stream, "lagrange_seg", grid_lanes(m), k_lagrange_seg, (const int32_t*)c->th.x.p, (const uint8_t*)c->status.p, m, (uint32_t)L.lo, goff + L.ga,
                 (uint32_t)(L.gb - L.ga), (uint32_t)TH_BATCH_TBIG, sigs ? (uint8_t*)nullptr : (uint8_t*)c->scalars.p + 32 * L.lo, (uint32_t*)c->th.glv.p, (uint32_t*)w.gid.p,
                 gstat + L.ga));
    }
    if (!sigs) continue;
    if (m) TRY(launch(c, c->stream, "g1_smul_glv", grid_lanes(m), k_g1_smul_glv, d_sigs + 64 * L.lo, (const uint32_t*)c->th.glv.p, (const uint32_t*)w.gid.p, m,
                      (int32_t*)w.pts.p, gstat + L.ga));
    TRY(seg_run_levels(w.seg, L.levels, {(const int32_t*)w.pts.p, m ? m : 1, nullptr}, {(int32_t*)w.gsum.p + L.ga, n_groups, nullptr},
                       [&](SegSrc in, const uint32_t* start, const uint32_t* len, size_t runs, SegDst out, bool) {
      return launch(c, c->stream, "g1_seg_sum", grid_lanes(runs), k_g1_seg_sum, in.v, in.stride, (const uint32_t*)nullptr, start, len, runs, out.v, out.stride);
    }));
  }
  if (sigs) TRY(launch(c, c->stream, "g1p_to_bytes", grid_lanes(n_groups), k_g1p_to_bytes, (const int32_t*)w.gsum.p, n_groups, n_groups, (uint8_t*)w.out.p));
  return launch(c, c->stream, "th_finish", grid_lanes(n_groups), k_th_finish, (const uint32_t*)gstat, n_groups, sigs ? (uint8_t*)w.out.p : (uint8_t*)nullptr, (uint8_t*)w.st.p);
}

// the same for ids (and partial signatures) of the caller: staged in c->in_b (c->in_a) first
static int th_enqueue(blsbn254_ctx* c, const uint8_t* ids, const uint8_t* sigs, const uint64_t* off, size_t n_groups) {
  const size_t N = (size_t)(off[n_groups] - off[0]), N1 = N ? N : 1;
  HIPCHK(c, c->in_b.reserve(32 * N1));
  if (sigs) HIPCHK(c, c->in_a.reserve(64 * N1));
  if (N) {
    HIPCHK(c, hipMemcpyAsync(c->in_b.p, ids + 32 * off[0], 32 * N, hipMemcpyHostToDevice, c->stream));
    if (sigs) HIPCHK(c, hipMemcpyAsync(c->in_a.p, sigs + 64 * off[0], 64 * N, hipMemcpyHostToDevice, c->stream));
  }
  return th_enqueue_dev(c, (const uint8_t*)c->in_b.p, sigs ? (const uint8_t*)c->in_a.p : nullptr, off, n_groups);
}

static int th_args(blsbn254_ctx* c, const uint8_t* ids, const uint8_t* second, bool need_second, const uint64_t* off, size_t n_groups, const void* out, const void* status) {
  if (!off || !status) return BLSBN254_E_ARG;
  if (check_offsets(off, n_groups)) { c->last_error = "group offsets decrease"; return BLSBN254_E_ARG; }
  const size_t N = (size_t)(off[n_groups] - off[0]);
  if (N && (!ids || !out || (need_second && !second))) return BLSBN254_E_ARG;
  if (need_second && !out) return BLSBN254_E_ARG;
  CHECK_LANES(c, N);
  CHECK_LANES(c, n_groups);
  return 0;
}

int blsbn254_threshold_combine_batch(blsbn254_ctx* c, const uint8_t* ids, const uint8_t* partial_sigs, const uint64_t* off, size_t n_groups,
                                     uint8_t* out_sigs, uint8_t* status) {
  if (!c) return BLSBN254_E_ARG;
  if (n_groups == 0) return 0;
  int rc = th_args(c, ids, partial_sigs, true, off, n_groups, out_sigs, status);
  if (rc) return rc;
  ENTER(c);
  rc = th_enqueue(c, ids, partial_sigs, off, n_groups);
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(out_sigs, c->thb.out.p, 64 * n_groups, hipMemcpyDeviceToHost, c->stream));
  TRY(download(c, status, c->thb.st.p, n_groups));
  // the large groups, one after the other through the single-group pipeline; their point check came from the lanes above
  for (size_t g = 0; g < n_groups; ++g) {
    const size_t t = (size_t)(off[g + 1] - off[g]);
    if (t <= TH_BATCH_TBIG) { ++c->thb.stat[0]; continue; }
    ++c->thb.stat[1];
    uint8_t* o = out_sigs + 64 * g;
    rc = threshold_combine_one(c, ids + 32 * off[g], partial_sigs + 64 * off[g], t, o);
    if (rc < 0) return rc;
    const uint8_t code = rc == BLSBN254_ERR_SCALAR ? BLSBN254_ERR_SCALAR : (rc == BLSBN254_ERR_G1 || status[g] == BLSBN254_ERR_G1) ? BLSBN254_ERR_G1 : 0;
    status[g] = code;
    if (code) g1_identity_bytes(o);
  }
  return 0;
}

int blsbn254_lagrange_at_zero_batch(blsbn254_ctx* c, const uint8_t* ids, const uint64_t* off, size_t n_groups, uint8_t* out, uint8_t* status) {
  if (!c) return BLSBN254_E_ARG;
  if (n_groups == 0) return 0;
  int rc = th_args(c, ids, nullptr, false, off, n_groups, out, status);
  if (rc) return rc;
  ENTER(c);
  rc = th_enqueue(c, ids, nullptr, off, n_groups);
  if (rc) return rc;
  const size_t N = (size_t)(off[n_groups] - off[0]);
  if (N) HIPCHK(c, hipMemcpyAsync(out, c->scalars.p, 32 * N, hipMemcpyDeviceToHost, c->stream));
  TRY(download(c, status, c->thb.st.p, n_groups));
  for (size_t g = 0; g < n_groups; ++g) {
    const size_t t = (size_t)(off[g + 1] - off[g]);
    uint8_t* o = out + 32 * (off[g] - off[0]);
    if (t <= TH_BATCH_TBIG) ++c->thb.stat[0];
    else {
      ++c->thb.stat[1];
      rc = lagrange_one(c, ids + 32 * off[g], t, o);
      if (rc < 0) return rc;
      status[g] = rc == BLSBN254_ERR_SCALAR ? BLSBN254_ERR_SCALAR : 0;
    }
    if (status[g]) std::memset(o, 0, 32 * t);            // the coefficients of a bad group: zero bytes
  }
  return 0;
}

int blsbn254_threshold_batch_stats(blsbn254_ctx* c, uint64_t out[4]) {
  TRY(COPY_STATS(c, thb.stat, 3, out));
  out[3] = TH_BATCH_TBIG;
  return 0;
}

}  // extern "C"
