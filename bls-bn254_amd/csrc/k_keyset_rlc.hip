// k_keyset_rlc.hip -- key-set FastAggregateVerify by random linear combination per message (keyset_rlc.h has the lane functions,
// keyset_rlc_plan.h the plan; host_keyset_rlc.hip).  The groups' key sums are in the sum path's buffers already:
//   k_ksr_elig       one lane per group: the eligibility byte (row ok, every added key has the KeyValidate bit, the signature
//                    decodes / is on the curve / is not the identity, the sum is not the identity) and the weight r_g.  The
//                    committee form tests the row against the committee's words instead of the registry's
//   k_ksr_weigh_g1   one lane per group: A = [r_g] sig_g, stored at the group's SORTED position (the identity when not eligible)
//   k_ksr_weigh_g2   the hot kernel, one lane per group: B = [r_g] S_g likewise.  Apart from G1 so that its registers hold one
//                    accumulator, the point and one sum, and nothing else.  A lane that is not eligible stores the identity and
//                    leaves: a wave of such lanes costs nothing
//   k_ksr_chunks     one lane per chunk, behind the segmented sums of A and B (k_g1_seg_sum, k_g2_seg_sum): the count of
//                    eligible members, the state (keyset_rlc.h) and the encoding of the chunk's G1 sum
//   k_ksr_gather     one lane per listed column: a G2 point, its flag and 64 signature bytes into compact buffers, for the
//                    sub-calls of the verify pipeline (the checked chunks; the groups of the exact list)
// Plain vector stores, no atomics; no lane reads what another lane of the same launch wrote.
#include "keyset_rlc.h"
#include "kernels.h"
using namespace bn;

__device__ inline void ksr_store_g1p(int32_t* ws, size_t stride, const G1P& p) {
  store_fp(ws, stride, p.x); store_fp(ws + NL * stride, stride, p.y); store_fp(ws + 2 * NL * stride, stride, p.z);
}

// rows: the call's rows; com == nullptr: the full-width form, row g at g * ceil(n_keys / 8), skip / valid the registry's words;
// else row g at row_off[g], as wide as committee com[g], skip / valid the table's words (at the committee's word base)
BN_KERNEL k_ksr_elig(const uint8_t* rows, const uint64_t* row_off, uint32_t n_keys, const uint32_t* com, const uint4* coms, const uint32_t* skip,
                     const uint32_t* valid, const int32_t* sums, const uint8_t* sum_ok, size_t G, const uint8_t* sigs, const uint8_t* seed,
                     const uint8_t* multi, uint8_t* elig, uint64_t* wt) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  bool e = false;
  uint64_t r = 1;
  if (multi[g]) {                                        // a chunk of one has nothing to combine with
    bool rv;
    if (com) {
      const uint4 k = coms[com[g]];                      // off, size, wbase
      rv = ksr_row_valid(rows + row_off[g], k.y, skip + k.z, valid + k.z);
    } else rv = ksr_row_valid(rows + g * ks_row_bytes(n_keys), n_keys, skip, valid);
    G1A sig;
    const bool so = ksr_sig_ok(sigs + 64 * g, sig);
    e = ksr_eligible(sum_ok[g] != 0, rv, so, ksr_is_identity(sums + g, G));
    r = ksr_weight(seed, (uint64_t)g, sigs + 64 * g);
  }
  elig[g] = e ? 1 : 0;
  wt[g] = r;
}

BN_KERNEL k_ksr_weigh_g1(const uint8_t* sigs, const uint8_t* elig, const uint64_t* wt, const uint32_t* pos, size_t G, int32_t* a_ws) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  int32_t* out = a_ws + pos[g];
  if (!elig[g]) { ksr_store_g1p(out, G, proj_identity<Fp>()); return; }
  bool ok;
  const G1A sig = g1_decode(sigs + 64 * g, ok);          // eligible: it decodes, is on the curve and is not the identity
  ksr_store_g1p(out, G, ksr_mul_u64(proj_from_affine(sig), wt[g]));
}

BN_KERNEL k_ksr_weigh_g2(const int32_t* sums, const uint8_t* elig, const uint64_t* wt, const uint32_t* pos, size_t G, int32_t* b_ws) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  int32_t* out = b_ws + pos[g];
  if (!elig[g]) { ks_store_point(out, G, proj_identity<Fp2>()); return; }
  ks_store_point(out, G, ksr_mul_u64(ks_load_point(sums + g, G), wt[g]));
}

// sa / sb: the chunks' sums (stride M)
BN_KERNEL k_ksr_chunks(const int32_t* sa, const int32_t* sb, size_t M, const uint32_t* cstart, const uint32_t* clen, const uint32_t* order,
                       const uint8_t* elig, uint32_t* cnt, uint8_t* state, uint8_t* sa_bytes) {
  const size_t ch = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= M) return;
  const uint32_t s0 = cstart[ch], len = clen[ch];
  uint32_t n = 0;
  for (uint32_t j = 0; j < len; ++j) n += elig[order[s0 + j]];
  const G1P A = {load_fp(sa + ch, M), load_fp(sa + NL * M + ch, M), load_fp(sa + 2 * NL * M + ch, M)};
  cnt[ch] = n;
  state[ch] = ksr_chunk_state(n, fp_is_zero(A.z), ksr_is_identity(sb + ch, M));
  g1_encode(sa_bytes + 64 * ch, g1_to_affine(A));
}

// column list[j] of pts (54 limbs, stride pts_stride) -> column j of c_pts (stride m); ok == nullptr: every flag is 1
__global__ void __launch_bounds__(256) k_ksr_gather(const uint32_t* list, size_t m, const int32_t* pts, size_t pts_stride, const uint8_t* ok, const uint8_t* sigs,
                                                   int32_t* c_pts, uint8_t* c_ok, uint8_t* c_sigs) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const size_t i = list[j];
  for (int k = 0; k < 6 * NL; ++k) c_pts[(size_t)k * m + j] = pts[(size_t)k * pts_stride + i];
  c_ok[j] = ok ? ok[i] : 1;
  const uint32_t* s = (const uint32_t*)(sigs + 64 * i);
  uint32_t* d = (uint32_t*)(c_sigs + 64 * j);
  for (int k = 0; k < 16; ++k) d[k] = s[k];
}
