// host_compressed.hip -- the entry points that take compressed encodings (64-byte G2 keys, 32-byte G1 signatures, as
// blsbn254_g1/g2_compress_batch write them).  One device stage, k_g1_inflate / k_g2_inflate (k_inflate.hip, inflate.h), turns
// every element into its uncompressed bytes or, when it does not decode, into the marker no decoder accepts -- per element,
// never an error of the call.  The compressed bytes are uploaded to wire_a / wire_b and inflated into in_a / in_b, the buffers
// the existing pipelines read: from there on each call here IS the uncompressed call's body (verify_batch_host,
// verify_batch_rlc_host, ks_create, ks_verify_rows), so chunking, limits and results are theirs and nothing but the bitmap
// comes back to the host.  Host side of include/blsbn254.h; see host_common.h.
#include "host_common.h"

extern "C" {

// n compressed elements at d_in inflated to d_out (status: a byte per element, or null), launch chunk by launch chunk
static int inflate_dev(blsbn254_ctx* c, const uint8_t* d_in, size_t n, uint8_t* d_out, uint8_t* d_status, bool g2) {
  return for_chunks(c, n, [&](size_t lo, size_t m) {
    uint8_t* st = d_status ? d_status + lo : nullptr;
    if (g2) return launch(c, c->stream, "g2_inflate", grid_lanes(m), k_g2_inflate, d_in + 64 * lo, m, d_out + 128 * lo, st);
    return launch(c, c->stream, "g1_inflate", grid_lanes(m), k_g1_inflate, d_in + 32 * lo, m, d_out + 64 * lo, st);
  });
}
int stage_g2(blsbn254_ctx* c, const uint8_t* pks, size_t n, bool compressed) {
  if (!compressed) return upload(c, c->in_a, pks, 128 * n);
  HIPCHK(c, c->in_a.reserve(128 * n));
  TRY(upload(c, c->wire_a, pks, 64 * n));
  return inflate_dev(c, (const uint8_t*)c->wire_a.p, n, (uint8_t*)c->in_a.p, nullptr, true);
}
int stage_g1(blsbn254_ctx* c, const uint8_t* sigs, size_t n, bool compressed) {
  if (!compressed) return upload(c, c->in_b, sigs, 64 * n);
  HIPCHK(c, c->in_b.reserve(64 * n));
  TRY(upload(c, c->wire_b, sigs, 32 * n));
  return inflate_dev(c, (const uint8_t*)c->wire_b.p, n, (uint8_t*)c->in_b.p, nullptr, false);
}

int g1_inflate_dev(blsbn254_ctx* c, const uint8_t* d_in, size_t n, uint8_t* d_out) { return inflate_dev(c, d_in, n, d_out, nullptr, false); }

// ---------------- the inflate primitives: the per-element form of blsbn254_g1/g2_decompress_batch
static int inflate_common(blsbn254_ctx* c, const uint8_t* in, size_t n, uint8_t* out, uint8_t* status, bool g2) {
  if (!c || (n && (!in || !out || !status))) return BLSBN254_E_ARG;
  if (n == 0) return 0;
  ENTER(c);
  const size_t full = g2 ? 128 : 64;
  HIPCHK(c, c->out.reserve(full * n)); HIPCHK(c, c->status.reserve(n));
  TRY(upload(c, g2 ? c->wire_a : c->wire_b, in, full / 2 * n));
  TRY(inflate_dev(c, (const uint8_t*)(g2 ? c->wire_a : c->wire_b).p, n, (uint8_t*)c->out.p, (uint8_t*)c->status.p, g2));
  HIPCHK(c, hipMemcpyAsync(out, c->out.p, full * n, hipMemcpyDeviceToHost, c->stream));
  return download(c, status, c->status.p, n);
}
int blsbn254_g1_inflate_batch(blsbn254_ctx* c, const uint8_t* in, size_t n, uint8_t* g1, uint8_t* status) { return inflate_common(c, in, n, g1, status, false); }
int blsbn254_g2_inflate_batch(blsbn254_ctx* c, const uint8_t* in, size_t n, uint8_t* g2, uint8_t* status) { return inflate_common(c, in, n, g2, status, true); }

// ---------------- verify
int blsbn254_verify_batch_compressed(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs,
                                     size_t n, const uint8_t* dst, size_t dst_len, uint8_t* bm) {
  if (!c || !off || (n && (!pks || !sigs || !bm)) || (dst_len && !dst)) return BLSBN254_E_ARG;
  if (n == 0) return 0;
  ENTER(c);
  return verify_batch_host(c, pks, msgs, off, sigs, n, dst, dst_len, bm, true);
}
int blsbn254_verify_batch_rlc_compressed(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs,
                                         size_t n, const uint8_t* dst, size_t dst_len, const uint8_t seed[32], uint8_t* bm) {
  if (!c || !off || (n && (!pks || !sigs || !bm)) || (dst_len && !dst)) return BLSBN254_E_ARG;
  if (n == 0) return 0;
  ENTER(c);
  return verify_batch_rlc_host(c, pks, msgs, off, sigs, n, dst, dst_len, seed, bm, true);
}

// ---------------- key sets
int blsbn254_keyset_create_compressed(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* proofs, size_t n_keys, const uint8_t* pop_dst, size_t pop_dst_len,
                                      blsbn254_keyset** out) {
  if (out) *out = nullptr;
  if (proofs && pop_dst_len && !pop_dst) return BLSBN254_E_ARG;
  return ks_create(c, pks, proofs, n_keys, proofs ? pop_dst : nullptr, proofs ? pop_dst_len : 0, out, true);
}
int blsbn254_keyset_fast_aggregate_verify_batch_compressed(blsbn254_ctx* c, const blsbn254_keyset* k, const uint8_t* sel, const uint8_t* msgs, const uint64_t* off,
                                                           const uint8_t* sigs, size_t n_groups, const uint8_t* dst, size_t dst_len, uint8_t* valid_bitmap) {
  if (!c || !k || k->ctx != c || !off || (n_groups && (!sel || !sigs || !valid_bitmap)) || (dst_len && !dst)) return BLSBN254_E_ARG;
  if (n_groups == 0) return 0;
  TRY(ks_args(c, k, sel, n_groups));
  ENTER(c);
  return ks_verify_rows(c, k, sel, msgs, off, sigs, n_groups, dst, dst_len, valid_bitmap, true);
}

}  // extern "C"
