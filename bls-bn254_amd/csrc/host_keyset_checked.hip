// host_keyset_checked.hip -- the body the four checked calls over a registered key set share: signature aggregation and merge
// of partial aggregates, over the whole registry (host_keyset_agg.hip, host_keyset_merge.hip) and per committee
// (host_keyset_committee_agg.hip, host_keyset_committee_merge.hip), each with 64-byte and with 32-byte signatures.  Those units
// keep their arguments, their own staging and their selection kernels; every step here is written once.  See host_common.h
// (CkWs, CkArgs) and DESIGN.md 6i.
//
// A call makes two attempts (ck_two_attempts), each ONE pass of enqueued work and one download:
//   optimistic   the form's kernels leave a candidate bit and a point per entry and a row per group; ck_tail sums the candidates'
//                signatures per group (k_g1_seg_sum by levels), sums the keys the rows name ON THE DEVICE (the form's callable) and
//                runs ONE verification per group of (key sum, message, signature sum).
//   fallback     only for groups that had a candidate and failed, their candidates repacked by the host into a sub-call: every
//                entry verified on its own (ck_verify_entries / ck_verify_contributions, the group's message once per entry),
//                then the SAME pass with those bits as the selection's mask -- so the kept entries are summed again and the one
//                equation decides.  No failing group: nothing is launched.
// A group's outcome depends on its own inputs only: which attempt served it, where a launch ended and how many groups shared
// the call do not change a byte.
#include "host_common.h"

extern "C" {

int ck_args(blsbn254_ctx* c, const blsbn254_keyset* k, const CkArgs& A, bool missing, bool ent_missing, bool committees, const char* noun) {
  if (!c) return BLSBN254_E_ARG;
  const auto bad = [&](const std::string& why) { c->last_error = why; return BLSBN254_E_ARG; };
  if (!k) return bad("a NULL argument");
  if (k->ctx != c) return bad("the key set belongs to another context");
  if (A.n_groups == 0) return CK_NOTHING;
  if (missing || !A.ent_off || !A.msg_off || (A.dst_len && !A.dst)) return bad("a NULL argument");
  if (committees && k->cm.tab.com.empty()) return bad("the key set has no committees (blsbn254_keyset_set_committees)");
  if (A.n_groups > c->chunk) return bad("more groups than one launch chunk");
  if (check_offsets(A.ent_off, A.n_groups)) return bad(std::string(noun) + " offsets decrease");
  if (check_offsets(A.msg_off, A.n_groups)) return bad("message offsets decrease");
  if (!A.msgs && A.msg_off[A.n_groups] != A.msg_off[0]) return bad("a NULL argument");
  if (A.ent_off[A.n_groups] != A.ent_off[0] && (ent_missing || !A.sigs)) return bad("a NULL argument");
  return 0;
}

int ck_stage_sigs(blsbn254_ctx* c, CkWs& w, const CkArgs& A, size_t N, bool inflate) {
  const uint64_t first = A.ent_off[0];
  if (!A.wire || inflate) HIPCHK(c, w.sigs.reserve(64 * (N ? N : 1)));
  if (!N) return 0;
  if (!A.wire) return upload(c, w.sigs, A.sigs + 64 * first, 64 * N);
  TRY(upload(c, w.wire, A.sigs + 32 * first, 32 * N));
  return inflate ? g1_inflate_dev(c, (const uint8_t*)w.wire.p, N, (uint8_t*)w.sigs.p) : 0;
}

int ck_reserve_key_sums(blsbn254_ctx* c, size_t n) {
  HIPCHK(c, c->gs.pk.reserve(128 * n)); HIPCHK(c, c->gs.sum.reserve(n * 54 * 4)); HIPCHK(c, c->gs.sum_ok.reserve(n));
  return 0;
}

void ck_expand_msgs(CkWs& w, const CkArgs& A) {
  w.s_emsgs.clear(); w.s_emoff.assign(1, 0);
  for (size_t g = 0; g < A.n_groups; ++g)
    for (uint32_t s = w.goff.h[g]; s < w.goff.h[g + 1]; ++s) {
      if (A.msg_off[g + 1] != A.msg_off[g]) w.s_emsgs.insert(w.s_emsgs.end(), A.msgs + A.msg_off[g], A.msgs + A.msg_off[g + 1]);
      w.s_emoff.push_back(w.s_emsgs.size());
    }
}

int ck_tail(blsbn254_ctx* c, CkWs& w, const CkArgs& A, uint32_t dl, const std::function<int()>& key_sums) {
  const size_t ng = A.n_groups, N = w.goff.h[ng], N1 = N ? N : 1;
  HIPCHK(c, w.gsum.reserve(27 * ng * 4)); HIPCHK(c, w.out.reserve(64 * ng)); HIPCHK(c, w.gbits.reserve((ng + 7) / 8 + 8));
  if (A.wire) HIPCHK(c, w.wout.reserve(32 * ng));
  // the signature sums: launches of whole groups, planned up front (a group has at most MAX_LANES entries)
  w.seg.h_start.clear(); w.seg.h_len.clear();
  std::vector<SegLaunch> launches;
  size_t m_max, items_max;
  if (!plan_launches_whole(w.goff.h, ng, c->chunk, CK_SUM_GROUP, (size_t)-1, launches, w.seg.h_start, w.seg.h_len, &m_max, &items_max)) {
    c->last_error = "internal: group sums do not converge";
    return BLSBN254_E_HIP;
  }
  TRY(seg_stage(c, w.seg, items_max, 27, false));
  for (const SegLaunch& L : launches)
    TRY(seg_run_levels(w.seg, L.levels, {(const int32_t*)w.pts.p + L.lo, N1, nullptr}, {(int32_t*)w.gsum.p + L.ga, ng, nullptr},
                       [&](SegSrc in, const uint32_t* start, const uint32_t* len, size_t runs, SegDst out, bool) {
      return launch(c, c->stream, "g1_seg_sum", grid_lanes(runs), k_g1_seg_sum, in.v, in.stride, (const uint32_t*)nullptr, start, len, runs, out.v, out.stride);
    }));
  if (A.wire) TRY(launch(c, c->stream, "g1p_to_wire", grid_lanes(ng), k_g1p_to_wire, (const int32_t*)w.gsum.p, ng, ng, (uint8_t*)w.out.p, (uint8_t*)w.wout.p));
  else TRY(launch(c, c->stream, "g1p_to_bytes", grid_lanes(ng), k_g1p_to_bytes, (const int32_t*)w.gsum.p, ng, ng, (uint8_t*)w.out.p));
  // the key sums from the rows where they are, then the equation of the fast aggregate verify over rows
  TRY(key_sums());
  TRY(launch(c, c->stream, "g2p_to_bytes", grid_lanes(ng), k_g2p_to_bytes, (const int32_t*)c->gs.sum.p, ng, (const uint8_t*)c->gs.sum_ok.p, ng, (uint8_t*)c->gs.pk.p, 1));
  TRY(stage_msgs(c, A.msgs, A.msg_off, ng));               // ONE message per group
  return verify_chunk_dev(c, (const uint8_t*)c->gs.pk.p, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, (const uint8_t*)w.out.p, ng, dl, (uint8_t*)w.gbits.p);
}

const uint64_t* ck_even_rows(CkWs& w, size_t n_groups, size_t row_bytes) {
  w.even_off.resize(n_groups + 1);
  for (size_t g = 0; g <= n_groups; ++g) w.even_off[g] = g * row_bytes;
  return w.even_off.data();
}

// what an attempt over ng groups left on the device, enqueued behind it: the sums as the caller gets them, the rows, the used
// bits of its n entries (merge forms) and, waited for, the bits of the groups' equation into w.h_gbits
static int ck_fetch(blsbn254_ctx* c, CkWs& w, bool wire, size_t ng, size_t row_bytes, size_t n, uint8_t* sigs, uint8_t* rows, bool used) {
  const size_t nb = (n + 7) / 8;
  w.h_gbits.assign((ng + 7) / 8, 0);
  HIPCHK(c, hipMemcpyAsync(sigs, wire ? w.wout.p : w.out.p, (wire ? 32 : 64) * ng, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(rows, w.orows.p, row_bytes, hipMemcpyDeviceToHost, c->stream));
  if (used) {
    w.h_used.assign(nb + 1, 0);
    if (nb) HIPCHK(c, hipMemcpyAsync(w.h_used.data(), w.used.p, nb, hipMemcpyDeviceToHost, c->stream));
  }
  return download(c, w.h_gbits.data(), w.gbits.p, (ng + 7) / 8);
}

int ck_two_attempts(blsbn254_ctx* c, CkWs& w, const CkArgs& A, const uint64_t* row_off, const CkOut& O, uint64_t stat[4],
                    const std::function<int(bool)>& attempt, const std::function<CkSub(const std::vector<size_t>&)>& repack) {
  const size_t ng = A.n_groups, sb = A.wire ? 32 : 64;
  const uint64_t first = A.ent_off[0], N = A.ent_off[ng] - first, nb = (N + 7) / 8;
  const auto row = [&](size_t g) { return O.rows + (row_off[g] - row_off[0]); };
  uint8_t* const used = O.used;                             // (locals: the byte stores below alias nothing the loops reload)
  TRY(attempt(false));
  if (used) {                                               // the merge forms' repack reads the candidate bitmap
    w.h_cand.assign(nb + 1, 0);
    if (nb) HIPCHK(c, hipMemcpyAsync(w.h_cand.data(), w.cand.p, nb, hipMemcpyDeviceToHost, c->stream));
    std::memset(used, 0, nb);
  }
  TRY(ck_fetch(c, w, A.wire, ng, row_off[ng] - row_off[0], N, O.sigs, O.rows, used));
  const uint8_t* h_used = w.h_used.data();
  // a group whose equation holds: its selected entries are used.  One whose equation does not hold: the identity and no used
  // bit -- and the fallback if its row shows that it had a candidate
  w.fail.clear();
  for (size_t g = 0; g < ng; ++g) {
    if (bit_at(w.h_gbits.data(), g)) {
      O.status[g] = 0; ++stat[0];
      if (used)
        for (uint64_t s = A.ent_off[g] - first, e = A.ent_off[g + 1] - first; s < e; ++s)
          if (bit_at(h_used, s)) used[s >> 3] |= (uint8_t)(1u << (s & 7));
      continue;
    }
    O.status[g] = BLSBN254_ST_SHORT;
    g1_identity_out(O.sigs + sb * g, A.wire);
    if (std::any_of(row(g), row(g + 1), [](uint8_t b) { return b != 0; })) w.fail.push_back(g);
    else ++stat[3];
  }
  if (w.fail.empty()) return 0;
  // the sub-call over the failing groups' candidates, repacked (ctx-owned: the arrays outlive the asynchronous uploads): its
  // messages first, so that the repack can point its call at them where they stay; the groups' rows are zero once the repack
  // has read them, and stay so unless the sub-call's equation holds
  const size_t nf = w.fail.size();
  w.s_msgs.clear(); w.s_moff.assign(1, 0);
  for (size_t g : w.fail) {
    if (A.msg_off[g + 1] != A.msg_off[g]) w.s_msgs.insert(w.s_msgs.end(), A.msgs + A.msg_off[g], A.msgs + A.msg_off[g + 1]);
    w.s_moff.push_back(w.s_msgs.size());
  }
  const CkSub S = repack(w.fail);
  for (size_t g : w.fail) std::memset(row(g), 0, row(g + 1) - row(g));
  stat[1] += nf; stat[2] += S.n;
  TRY(attempt(true));
  w.s_out.resize(sb * nf); w.s_rows.resize(S.row_off[nf] - S.row_off[0]);
  TRY(ck_fetch(c, w, A.wire, nf, w.s_rows.size(), S.n, w.s_out.data(), w.s_rows.data(), used));
  h_used = w.h_used.data();
  for (size_t j = 0; j < nf; ++j) {
    const size_t g = w.fail[j];
    if (!bit_at(w.h_gbits.data(), j)) { ++stat[3]; continue; }
    O.status[g] = 0;
    std::memcpy(O.sigs + sb * g, w.s_out.data() + sb * j, sb);
    std::memcpy(row(g), w.s_rows.data() + (S.row_off[j] - S.row_off[0]), row(g + 1) - row(g));
    if (!used) continue;
    for (uint64_t i = S.off[j]; i < S.off[j + 1]; ++i)
      if (bit_at(h_used, i)) { const uint64_t s = S.pos[i] - first; used[s >> 3] |= (uint8_t)(1u << (s & 7)); }
  }
  return 0;
}

int ck_verify_entries(blsbn254_ctx* c, const blsbn254_keyset* k, CkWs& w, DevBuf& pks, const uint32_t* d_idx, const CkArgs& A, size_t N) {
  // every entry as the tuple (its key, the group's message, its signature): the keys by index from the handle
  HIPCHK(c, pks.reserve(128 * N)); HIPCHK(c, w.vbits.reserve((N + 7) / 8 + 8));
  TRY(for_chunks(c, N, [&](size_t lo, size_t m) {
    return launch(c, c->stream, "ka_gather_keys", grid_lanes(8 * m), k_ka_gather_keys, (const uint4*)k->enc.p, d_idx + lo, m, (uint4*)pks.p + 8 * lo);
  }));
  ck_expand_msgs(w, A);
  TRY(stage_msgs(c, w.s_emsgs.data(), w.s_emoff.data(), N));
  return blsbn254_internal_verify_batch_dev_sync(c, (const uint8_t*)pks.p, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, (const uint8_t*)w.sigs.p, N, A.dst, A.dst_len,
                                                 (uint8_t*)w.vbits.p);
}

int ck_select(blsbn254_ctx* c, KmStage& w, size_t n_groups, size_t N, const std::function<int(size_t, size_t)>& select) {
  const size_t N1 = N ? N : 1, nb = (N + 7) / 8;
  HIPCHK(c, w.sig_ok.reserve(N1)); HIPCHK(c, w.flags.reserve(N1)); HIPCHK(c, w.used.reserve(nb + 8)); HIPCHK(c, w.cand.reserve(nb + 8));
  HIPCHK(c, w.pts.reserve(27 * N1 * 4));
  TRY(for_chunks(c, N, [&](size_t lo, size_t m) {
    return launch(c, c->stream, "km_sig", grid_lanes(m), k_km_sig, (const uint8_t*)w.sigs.p, m, (uint32_t)lo, N, (uint8_t*)w.sig_ok.p, (int32_t*)w.pts.p);
  }));
  // (the signature bytes are complete: every launch of the test is enqueued before the first group is walked)  A wave per group:
  // a launch of c->chunk lanes walks c->chunk / 64 groups
  const size_t Gl = std::max((size_t)1, c->chunk / 64);
  for (size_t lo = 0; lo < n_groups; lo += Gl) TRY(select(lo, std::min(Gl, n_groups - lo)));
  return for_chunks(c, N, [&](size_t lo, size_t m) {
    return launch(c, c->stream, "km_points", grid_lanes(m), k_km_points, (const uint8_t*)w.flags.p, m, (uint32_t)lo, N, (int32_t*)w.pts.p, (uint8_t*)w.used.p,
                  (uint8_t*)w.cand.p);
  });
}

int ck_verify_contributions(blsbn254_ctx* c, KmStage& w, const CkArgs& A, size_t N, uint32_t dl, bool settle,
                            const std::function<int(size_t, size_t)>& key_sums) {
  // every contribution as the tuple (the key sum of its row, the group's message, its signature), by launches of at most
  // c->chunk contributions.  settle (the committee form): the plan of a launch's key sums lives in c->kcom and the next launch
  // (or the groups' equation after it) plans over it, so a launch is settled before the next one is planned
  HIPCHK(c, w.vbits.reserve((N + 7) / 8 + 8));
  ck_expand_msgs(w, A);
  return for_chunks(c, N, [&](size_t lo, size_t m) {
    TRY(key_sums(lo, m));
    TRY(launch(c, c->stream, "g2p_to_bytes", grid_lanes(m), k_g2p_to_bytes, (const int32_t*)c->gs.sum.p, m, (const uint8_t*)c->gs.sum_ok.p, m, (uint8_t*)c->gs.pk.p, 1));
    TRY(stage_msgs(c, w.s_emsgs.data(), w.s_emoff.data() + lo, m));
    TRY(verify_chunk_dev(c, (const uint8_t*)c->gs.pk.p, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, (const uint8_t*)w.sigs.p + 64 * lo, m, dl,
                         (uint8_t*)w.vbits.p + (lo >> 3)));
    if (settle) HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
  });
}

}  // extern "C"
