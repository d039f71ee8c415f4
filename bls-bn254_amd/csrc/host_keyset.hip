// host_keyset.hip -- a registered set of public keys and the sums over it selected by participation bitmaps: impl Sum for
// G2Projective (g2.rs:579-583) and FastAggregateVerify over the subset of a committee a bitmap names.  The keys are uploaded,
// decoded and curve-checked ONCE (blsbn254_keyset_create); a call then carries one bit per (group, key) instead of 128 bytes,
// and a group in which more than half of the set signed is summed through its complement, total - sum of the unselected keys.
// Host side of include/blsbn254.h; kernels in k_keyset.hip, lane functions and layout in keyset.h; see host_common.h.
#include "host_common.h"

extern "C" {

static const size_t KS_MAX_KEYS = (size_t)1 << 16;
static const size_t KS_LAUNCH_ITEMS = (size_t)1 << 20;      // word partials of one launch: 54 x 4 B each, about 226 MB
static_assert(KS_LAUNCH_ITEMS == KC_LAUNCH_PARTIALS, "keyset_committee_plan.h cuts its launches by the same bound");
static const size_t KS_RUN_ITEMS = 16;                      // keyset.h KS_RUN
static inline size_t ks_nwords(size_t n) { return (n + 31) / 32; }

// The registration, with proofs of possession or without (proofs == nullptr: nothing below differs from a registration that
// never heard of them).  With proofs the pipeline of blsbn254_pop_verify_batch runs FIRST, on the staged keys and proofs: it owns
// the context's staging buffers while it runs and leaves in_a, the staged keys, as they were.  Its bits are kept on the handle
// and make a failing key bad (k_ks_register); for the total the same kernel overwrites the STAGED copy of such a key with an
// encoding that does not decode, after the handle's copy of the encodings was taken: enc keeps the bytes as uploaded.
// compressed: the keys (and the proofs) are wire encodings, inflated on the way into the staging buffers (stage_g2 / stage_g1):
// from there on nothing differs, so the handle is the one the inflated bytes would have made -- enc keeps the INFLATED bytes, a
// proof's message is the 128-byte uncompressed key, a key that does not inflate is the marker, which does not decode.
int ks_create(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* proofs, size_t n_keys, const uint8_t* pop_dst, size_t pop_dst_len,
              blsbn254_keyset** out, bool compressed) {
  if (!c || !out) return BLSBN254_E_ARG;
  *out = nullptr;
  if (!pks || n_keys == 0) return BLSBN254_E_ARG;
  if (n_keys > KS_MAX_KEYS) { c->last_error = "more than 65536 keys in one key set"; return BLSBN254_E_ARG; }
  ENTER(c);
  // owned until handed to the caller: every failure path below frees the object and, with it, its device buffers
  struct Owner { blsbn254_keyset* p; ~Owner() { delete p; } } own{new blsbn254_keyset()};
  blsbn254_keyset* k = own.p;
  k->ctx = c; k->n = n_keys;
  const size_t W = ks_nwords(n_keys);
  HIPCHK(c, k->aff.reserve(36 * n_keys * 4)); HIPCHK(c, k->bad.reserve(W * 4)); HIPCHK(c, k->skip.reserve(W * 4));
  HIPCHK(c, k->total.reserve(54 * 4)); HIPCHK(c, k->valid.reserve(n_keys)); HIPCHK(c, c->sub_ok.reserve(n_keys)); HIPCHK(c, k->enc.reserve(128 * n_keys));
  TRY(stage_g2(c, pks, n_keys, compressed));
  if (proofs) {
    const size_t nb = (n_keys + 7) / 8;
    HIPCHK(c, k->pop.reserve(nb + 8)); HIPCHK(c, c->in_off.reserve(8 * (n_keys + 1))); HIPCHK(c, c->bitmap.reserve(nb + 8));
    TRY(stage_g1(c, proofs, n_keys, compressed));
    TRY(launch(c, c->stream, "iota_off", grid_lanes(n_keys + 1), k_iota_off, (uint64_t*)c->in_off.p, n_keys, (uint64_t)128));
    RfcMapScope rfc(c);                                    // proofs of possession keep the RFC map and their tag (host_common.h)
    TRY(blsbn254_internal_verify_batch_dev_sync(c, (const uint8_t*)c->in_a.p, (const uint8_t*)c->in_a.p, (const uint64_t*)c->in_off.p,
                                                (const uint8_t*)c->in_b.p, n_keys, pop_dst, pop_dst_len, (uint8_t*)c->bitmap.p));
    HIPCHK(c, hipMemcpyAsync(k->pop.p, c->bitmap.p, nb, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, c->sub_ok.reserve(n_keys));                  // the pipeline above may have grown it for a size of its own
    k->checked = true;
  }
  const uint8_t* mask = proofs ? (const uint8_t*)k->pop.p : nullptr;
  HIPCHK(c, hipMemcpyAsync(k->enc.p, c->in_a.p, 128 * n_keys, hipMemcpyDeviceToDevice, c->stream));
  TRY(launch(c, c->stream, "g2_check", grid_lanes(n_keys), k_g2_check, (const uint8_t*)c->in_a.p, n_keys, (uint8_t*)c->sub_ok.p, (uint8_t*)nullptr));
  TRY(launch(c, c->stream, "ks_register", grid_lanes(n_keys), k_ks_register, (uint8_t*)c->in_a.p, (uint32_t)n_keys, (const uint8_t*)c->sub_ok.p, mask,
             (int32_t*)k->aff.p, (uint32_t*)k->bad.p, (uint32_t*)k->skip.p, (uint8_t*)k->valid.p));
  // the total: k_g2_load stores a bad key as the identity, and adding an identity key changes nothing, so the sum of ALL the
  // encodings is the sum of the non-skipped keys (the flag of that sum is not looked at)
  const uint64_t goff[2] = {0, (uint64_t)n_keys};
  TRY(g2_group_sums(c, (const uint8_t*)c->in_a.p, n_keys, goff, 1));
  HIPCHK(c, hipMemcpyAsync(k->total.p, c->gs.sum.p, 54 * 4, hipMemcpyDeviceToDevice, c->stream));
  // the KeyValidate bits by words, for the selection of the checked merge: packed once, here
  HIPCHK(c, k->vwords.reserve(W * 4));
  HIPCHK(c, hipMemsetAsync(k->vwords.p, 0, W * 4, c->stream));
  TRY(launch(c, c->stream, "pack_bitmap", grid_lanes(n_keys), k_pack_bitmap, (const uint8_t*)k->valid.p, n_keys, (uint8_t*)k->vwords.p));
  hipError_t es = hipStreamSynchronize(c->stream);
  if (es != hipSuccess) { (void)hipDeviceSynchronize(); }       // nothing may still be writing the buffers the owner frees
  HIPCHK(c, es);
  ++c->kset.stat[3];
  own.p = nullptr;
  *out = k;
  return 0;
}
int blsbn254_keyset_create(blsbn254_ctx* c, const uint8_t* pks, size_t n_keys, blsbn254_keyset** out) {
  return ks_create(c, pks, nullptr, n_keys, nullptr, 0, out, false);
}
int blsbn254_keyset_create_checked(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* proofs, size_t n_keys, const uint8_t* pop_dst, size_t pop_dst_len,
                                   blsbn254_keyset** out) {
  if (out) *out = nullptr;
  if (!proofs || (pop_dst_len && !pop_dst)) return BLSBN254_E_ARG;
  return ks_create(c, pks, proofs, n_keys, pop_dst, pop_dst_len, out, false);
}
int blsbn254_keyset_checked(const blsbn254_keyset* k) { return k && k->checked ? 1 : 0; }
void blsbn254_keyset_destroy(blsbn254_keyset* k) {
  if (!k) return;
  (void)hipSetDevice(k->ctx->device);
  (void)hipStreamSynchronize(k->ctx->stream);
  delete k;
}
size_t blsbn254_keyset_count(const blsbn254_keyset* k) { return k ? k->n : 0; }
// KeyValidate per registered key: decodes, not the identity, on the curve, in the r-torsion
int blsbn254_keyset_valid(blsbn254_ctx* c, const blsbn254_keyset* k, uint8_t* ok_bitmap) {
  if (!c || !k || k->ctx != c || !ok_bitmap) return BLSBN254_E_ARG;
  ENTER(c);
  HIPCHK(c, c->bitmap.reserve((k->n + 7) / 8 + 8));
  TRY(launch(c, c->stream, "pack_bitmap", grid_lanes(k->n), k_pack_bitmap, (const uint8_t*)k->valid.p, k->n, (uint8_t*)c->bitmap.p));
  return download(c, ok_bitmap, c->bitmap.p, (k->n + 7) / 8);
}

// the argument checks the calls over rows share (n_groups > 0): the limit, and no row may set a bit that names no key
int ks_args(blsbn254_ctx* c, const blsbn254_keyset* k, const uint8_t* sel, size_t n_groups) {
  if (n_groups > c->chunk) { c->last_error = "more groups than one launch chunk"; return BLSBN254_E_ARG; }
  const size_t rb = (k->n + 7) / 8;
  if (k->n & 7) {
    const uint8_t pad = (uint8_t)(0xffu << (k->n & 7));
    for (size_t g = 0; g < n_groups; ++g)
      if (sel[g * rb + rb - 1] & pad) { c->last_error = "row " + std::to_string(g) + " sets a bit past the last key"; return BLSBN254_E_ARG; }
  }
  return 0;
}
// The sums of every row (d_rows: on the device) into c->gs.sum / c->gs.sum_ok (enqueued), the flip bytes into c->kset.h_flip
// (enqueued: read after the caller's synchronising download).  A launch covers as many groups as keep groups x W within
// KS_LAUNCH_ITEMS partials (within ctx->chunk when that is smaller); launch starts are multiples of 8 groups.
int ks_enqueue_sums_dev(blsbn254_ctx* c, const blsbn254_keyset* k, const uint8_t* d_rows, size_t n_groups, size_t* launches) {
  KsetWs& w = c->kset;
  const size_t W = ks_nwords(k->n), rb = (k->n + 7) / 8;
  const size_t Gl = std::max((size_t)8, (std::min(KS_LAUNCH_ITEMS, c->chunk) / W) & ~(size_t)7), Gmax = std::min(Gl, n_groups);
  const size_t runs0 = (W + KS_RUN_ITEMS - 1) / KS_RUN_ITEMS;
  HIPCHK(c, w.flip.reserve(n_groups)); HIPCHK(c, w.ok.reserve(n_groups));
  HIPCHK(c, w.part[0].reserve(54 * 4 * W * Gmax)); HIPCHK(c, w.part[1].reserve(54 * 4 * runs0 * Gmax));
  HIPCHK(c, c->gs.sum.reserve(n_groups * 54 * 4)); HIPCHK(c, c->gs.sum_ok.reserve(n_groups));
  *launches = 0;
  for (size_t lo = 0; lo < n_groups; lo += Gl, ++*launches) {
    const size_t m = std::min(Gl, n_groups - lo);
    const uint8_t *flip = (const uint8_t*)w.flip.p + lo, *ok = (const uint8_t*)w.ok.p + lo, *rows = d_rows + lo * rb;
    TRY(launch(c, c->stream, "ks_count", grid_lanes(m), k_ks_count, rows, m, (uint32_t)k->n, (const uint32_t*)k->bad.p, (uint8_t*)w.flip.p + lo, (uint8_t*)w.ok.p + lo));
    TRY(launch(c, c->stream, "ks_word_sum", Shape{dim3(nblocks(m), (unsigned)W), dim3(256)}, k_ks_word_sum, (const int32_t*)k->aff.p, (uint32_t)k->n,
               (const uint32_t*)k->skip.p, rows, flip, m, (int32_t*)w.part[0].p, W * m));
    int src = 0;
    for (size_t cnt = W;;) {
      const size_t runs = (cnt + KS_RUN_ITEMS - 1) / KS_RUN_ITEMS;
      const bool last = runs == 1;
      TRY(launch(c, c->stream, "ks_group_sum", grid_lanes(runs * m), k_ks_group_sum, (const int32_t*)w.part[src].p, cnt * m, (uint32_t)cnt, m, flip, ok,
                 (const int32_t*)k->total.p, last ? 1 : 0, last ? (int32_t*)c->gs.sum.p + lo : (int32_t*)w.part[src ^ 1].p, last ? n_groups : runs * m,
                 last ? (uint8_t*)c->gs.sum_ok.p + lo : (uint8_t*)nullptr));
      if (last) break;
      src ^= 1; cnt = runs;
    }
  }
  w.h_flip.resize(n_groups);
  HIPCHK(c, hipMemcpyAsync(w.h_flip.data(), w.flip.p, n_groups, hipMemcpyDeviceToHost, c->stream));
  return 0;
}
// the same for rows of the caller: staged in c->kset.sel first
int ks_enqueue_sums(blsbn254_ctx* c, const blsbn254_keyset* k, const uint8_t* sel, size_t n_groups, size_t* launches) {
  TRY(upload(c, c->kset.sel, sel, (k->n + 7) / 8 * n_groups));
  return ks_enqueue_sums_dev(c, k, (const uint8_t*)c->kset.sel.p, n_groups, launches);
}
// counted once the call has succeeded (and synchronised: the flip bytes are on the host)
void ks_tally(blsbn254_ctx* c, size_t n_groups, size_t launches) {
  c->kset.stat[0] += n_groups; c->kset.stat[2] += launches;
  for (size_t g = 0; g < n_groups; ++g) c->kset.stat[1] += c->kset.h_flip[g] ? 1 : 0;
}

// row g: out = blsbn254_aggregate_pks on the selected keys in index order, status 1; a row that selects a key that does not
// decode or is off the curve: the identity encoding, status 0
int blsbn254_keyset_sum_batch(blsbn254_ctx* c, const blsbn254_keyset* k, const uint8_t* sel, size_t n_groups, uint8_t* out, uint8_t* status) {
  if (!c || !k || k->ctx != c || (n_groups && (!sel || !out || !status))) return BLSBN254_E_ARG;
  if (n_groups == 0) return 0;
  TRY(ks_args(c, k, sel, n_groups));
  ENTER(c);
  size_t launches;
  TRY(ks_enqueue_sums(c, k, sel, n_groups, &launches));
  HIPCHK(c, c->out.reserve(128 * n_groups));
  TRY(launch(c, c->stream, "g2p_to_bytes", grid_lanes(n_groups), k_g2p_to_bytes, (const int32_t*)c->gs.sum.p, n_groups, (const uint8_t*)c->gs.sum_ok.p, n_groups,
             (uint8_t*)c->out.p, 0));
  HIPCHK(c, hipMemcpyAsync(out, c->out.p, 128 * n_groups, hipMemcpyDeviceToHost, c->stream));
  TRY(download(c, status, c->gs.sum_ok.p, n_groups));
  ks_tally(c, n_groups, launches);
  return 0;
}

// from the groups' sums on (c->gs.sum / c->gs.sum_ok, enqueued; c->gs.pk and c->bitmap reserved by the caller): the pipeline of
// blsbn254_fast_aggregate_verify_batch.  Shared with the committee form (host_keyset_committee.hip).
int ks_verify_sums(blsbn254_ctx* c, size_t n_groups, uint32_t dl, uint8_t* valid_bitmap) {
  TRY(launch(c, c->stream, "g2p_to_bytes", grid_lanes(n_groups), k_g2p_to_bytes, (const int32_t*)c->gs.sum.p, n_groups, (const uint8_t*)c->gs.sum_ok.p, n_groups,
             (uint8_t*)c->gs.pk.p, 1));
  TRY(verify_chunk_dev(c, (const uint8_t*)c->gs.pk.p, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, (const uint8_t*)c->in_b.p, n_groups, dl,
                       (uint8_t*)c->bitmap.p));
  return download(c, valid_bitmap, c->bitmap.p, (n_groups + 7) / 8);
}
// bit g = blsbn254_fast_aggregate_verify_batch on the selected keys of row g: from the sums on, the same pipeline.  sel == nullptr:
// the rows are staged in c->kset.sel already (the verify with a quorum has weighed them there)
int ks_verify_rows(blsbn254_ctx* c, const blsbn254_keyset* k, const uint8_t* sel, const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs, size_t n_groups,
                   const uint8_t* dst, size_t dst_len, uint8_t* valid_bitmap, bool compressed) {
  uint32_t dl;
  TRY(stage_dst(c, dst, dst_len, &dl));
  TRY(stage_msgs(c, msgs, off, n_groups));
  const size_t nb = (n_groups + 7) / 8;
  HIPCHK(c, c->gs.pk.reserve(128 * n_groups)); HIPCHK(c, c->bitmap.reserve(nb + 8));
  TRY(stage_g1(c, sigs, n_groups, compressed));
  size_t launches;
  if (sel) TRY(ks_enqueue_sums(c, k, sel, n_groups, &launches));
  else TRY(ks_enqueue_sums_dev(c, k, (const uint8_t*)c->kset.sel.p, n_groups, &launches));
  TRY(ks_verify_sums(c, n_groups, dl, valid_bitmap));
  ks_tally(c, n_groups, launches);
  return 0;
}
int blsbn254_keyset_fast_aggregate_verify_batch(blsbn254_ctx* c, const blsbn254_keyset* k, const uint8_t* sel, const uint8_t* msgs, const uint64_t* off,
                                                const uint8_t* sigs, size_t n_groups, const uint8_t* dst, size_t dst_len, uint8_t* valid_bitmap) {
  if (!c || !k || k->ctx != c || !off || (n_groups && (!sel || !sigs || !valid_bitmap)) || (dst_len && !dst)) return BLSBN254_E_ARG;
  if (n_groups == 0) return 0;
  TRY(ks_args(c, k, sel, n_groups));
  ENTER(c);
  return ks_verify_rows(c, k, sel, msgs, off, sigs, n_groups, dst, dst_len, valid_bitmap);
}

int blsbn254_keyset_stats(blsbn254_ctx* c, uint64_t out[4]) { return COPY_STATS(c, kset.stat, 4, out); }

}  // extern "C"
