// k_aggregate_rlc.hip -- aggregate verify over ragged groups by random linear combination (aggregate_rlc.h has the lane functions,
// aggregate_rlc_plan.h the plan; host_aggregate_rlc.hip).  The weighted points of a call live in ONE limb-major
// workspace of W = N + G + V_max columns that key_sums reads: columns 0 .. N - 1 the pairs' r_g H_gi, N .. N + G - 1 the groups'
// r_g sig_g, then one identity per virtual key (key_sums wants no key without an item).
//   k_agr_group       one lane per group: the signature flag, the AND of its keys' validity by batch key id (a loop over the
//                     group's pairs: a lane per group is the shape of the call, groups are short), the eligibility byte (at least
//                     one pair, signature decodes / on the curve / not the identity, every key valid), the weight (a, b) and
//                     r_g sig_g, the identity when not eligible
//   k_agr_weigh       the hot kernel, one lane per TWO pairs (t and t + ceil(N / 2): both loads coalesce): r_g H_gi by the 32-step
//                     joint double-and-add, the two chains interleaved as in k_rlc2_prep; the identity for a pair of an ineligible
//                     group, by selection: the wave does not branch on eligibility.  No inversion
//   k_agr_items       one lane per item of a round: a pair's or a signature's virtual key id (segment * u + key id; S u + segment);
//                     for a virtual key its identity column, its id, and the table it pairs with (its key's; -G2gen's, table
//                     u, for a signature slot)
//   k_agr_bits        one lane per group: valid = eligible and its segment's product is one
// Plain vector stores, no atomics; no lane reads what another lane of the same launch wrote.
#include "aggregate_rlc.h"
#include "kernels.h"
using namespace bn;

// goff: the groups' pair offsets rebased to 0 (G + 1 entries); w_ws: the workspace, column col0 + g is the group's (stride W)
BN_KERNEL k_agr_group(const uint8_t* sigs, const uint32_t* goff, const uint32_t* kid, const uint8_t* key_ok, const uint8_t* seed, size_t G, uint8_t* sig_ok,
                      uint8_t* elig, uint2* wt, int32_t* w_ws, size_t W, size_t col0) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  G1A sig;
  const bool so = agr_sig_ok(sigs + 64 * g, sig);
  const uint32_t p0 = goff[g], p1 = goff[g + 1];
  uint8_t keys = 1;
#pragma unroll 1
  for (uint32_t i = p0; i < p1; ++i) keys &= key_ok[kid[i]];
  const bool e = so & (p1 > p0) & (keys != 0);
  const AgrWeight w = agr_weight(seed, (uint64_t)g, sigs + 64 * g);
  const G1P A = agr_mul_glv32(proj_from_affine(sig), w.a, w.b);
  agr_store_point(w_ws + col0 + g, W, proj_select(e, A, proj_identity<Fp>()));
  sig_ok[g] = so ? 1 : 0;
  elig[g] = e ? 1 : 0;
  wt[g] = make_uint2(w.a, w.b);
}

// h_ws: the homogeneous hash points of k_hash_to_g1 mode 3 (stride N); gidx: the group of every pair
BN_KERNEL k_agr_weigh(const int32_t* h_ws, size_t N, const uint32_t* gidx, const uint8_t* elig, const uint2* wt, int32_t* w_ws, size_t W) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, H = (N + 1) / 2;
  if (t >= H) return;
  const bool two = t + H < N;
  const size_t i0 = t, i1 = two ? t + H : t;             // an odd N: the last lane weighs its one pair twice and stores it once
  const uint32_t g0 = gidx[i0], g1 = gidx[i1];
  const uint2 w0 = wt[g0], w1 = wt[g1];
  G1P r0, r1;
  agr_mul_glv32_x2(agr_load_point(h_ws + i0, N), AgrWeight{w0.x, w0.y}, agr_load_point(h_ws + i1, N), AgrWeight{w1.x, w1.y}, r0, r1);
  const G1P id = proj_identity<Fp>();
  agr_store_point(w_ws + i0, W, proj_select(elig[g0] != 0, r0, id));
  if (two) agr_store_point(w_ws + i1, W, proj_select(elig[g1] != 0, r1, id));
}

// seg_of == nullptr: one segment (round 1).  Items: N pairs, G signatures, then the V = S (u + 1) virtual keys' identities
__global__ void __launch_bounds__(256) k_agr_items(const uint32_t* gidx, const uint32_t* kid, const uint32_t* seg_of, size_t N, size_t G, uint32_t u, uint32_t S,
                                                  int32_t* w_ws, size_t W, uint32_t* vkid, uint32_t* mkid) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, V = (size_t)S * (u + 1);
  if (i >= N + G + V) return;
  if (i < N + G) {
    const uint32_t s = seg_of ? seg_of[i < N ? gidx[i] : i - N] : 0u;
    vkid[i] = i < N ? s * u + kid[i] : S * u + s;
    return;
  }
  const uint32_t v = (uint32_t)(i - (N + G));
  agr_store_point(w_ws + i, W, proj_identity<Fp>());
  vkid[i] = v;
  mkid[v] = v < S * u ? v % u : u;
}

__global__ void __launch_bounds__(256) k_agr_bits(const uint8_t* elig, const uint32_t* seg_of, const uint8_t* isone, size_t G, uint8_t* valid) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  valid[g] = (elig[g] != 0 && isone[seg_of ? seg_of[g] : 0] != 0) ? 1 : 0;
}
