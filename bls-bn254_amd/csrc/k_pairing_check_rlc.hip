// k_pairing_check_rlc.hip -- pairing-product checks over ragged groups by random linear combination (pairing_check_rlc.h has the
// lane functions, pairing_check_rlc_plan.h the plan; host_pairing_check_rlc.hip).  The weighted points of a call live
// in ONE limb-major workspace of W = N + V_max columns that key_sums reads: columns 0 .. N - 1 the pairs' r_g P_gj, then one
// identity per virtual key (key_sums wants no key without an item).
//   k_pcr_pairs       one lane per pair: its byte (PCR_OK, PCR_SKIP) from the decoded P, P's curve equation, Q's identity by its
//                     encoding and key_ok[kid[i]] of the DISTINCT Q's preparation; the decoded P (a stand-in where the pair is
//                     skipped or not OK) as affine limbs for k_pcr_weigh: no point is decoded twice, no torsion test runs here
//   k_pcr_eq          one lane per equation: the AND of its pairs' OK bits (a loop over the equation's pairs, one byte each: a
//                     lane per equation is the shape of the call; an equation of 2^20 pairs is 2^20 dependent-free byte loads in
//                     one lane), the eligibility byte and the weight (a, b)
//   k_pcr_weigh       the hot kernel, one lane per TWO pairs (t and t + ceil(N / 2): both loads coalesce): r_g P_gj by the 32-step
//                     joint double-and-add over affine entries (mixed additions), the two chains interleaved; the identity for a
//                     skipped pair or a pair of an ineligible equation, by selection: the wave does not branch.  No inversion.
//                     -DPCR_WEIGH_PLAIN (measurement builds): agr_mul_glv32_x2 on z = 1 in its place
//   k_pcr_items       one lane per item of a round: a pair's virtual key id (segment * u + key id); for a virtual key its identity
//                     column, its id, and the table it pairs with (its Q's).  k_agr_items without the signature slots
// The final bits are k_agr_bits'.  Plain vector stores, no atomics; no lane reads what another lane of the same launch wrote.
#include "pairing_check_rlc.h"
#include "kernels.h"
using namespace bn;

// p_ws: 18 x N limbs (x, y), stride N
BN_KERNEL k_pcr_pairs(const uint8_t* g1, const uint8_t* g2, const uint32_t* kid, const uint8_t* key_ok, size_t N, int32_t* p_ws, uint8_t* flag) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  G1A p;
  flag[i] = pcr_pair(g1 + 64 * i, g2 + 128 * i, key_ok[kid[i]], p);
  pcr_store_affine(p_ws + i, N, p);
}

// goff: the equations' pair offsets rebased to 0 (G + 1 entries)
BN_KERNEL k_pcr_eq(const uint32_t* goff, const uint8_t* flag, const uint8_t* seed, size_t G, uint8_t* elig, uint2* wt) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const bool ok = pcr_eligible(flag, goff[g], goff[g + 1]);
  const AgrWeight w = pcr_weight(seed, (uint64_t)g);
  elig[g] = ok ? 1 : 0;
  wt[g] = make_uint2(w.a, w.b);
}

BN_KERNEL k_pcr_weigh(const int32_t* p_ws, size_t N, const uint32_t* gidx, const uint8_t* flag, const uint8_t* elig, const uint2* wt, int32_t* w_ws, size_t W) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, H = (N + 1) / 2;
  if (t >= H) return;
  const bool two = t + H < N;
  const size_t i0 = t, i1 = two ? t + H : t;             // an odd N: the last lane weighs its one pair twice and stores it once
  const uint32_t g0 = gidx[i0], g1 = gidx[i1];
  const uint2 w0 = wt[g0], w1 = wt[g1];
  G1P r0, r1;
#ifdef PCR_WEIGH_PLAIN
  agr_mul_glv32_x2(proj_from_affine(pcr_load_affine(p_ws + i0, N)), AgrWeight{w0.x, w0.y}, proj_from_affine(pcr_load_affine(p_ws + i1, N)), AgrWeight{w1.x, w1.y}, r0, r1);
#else
  pcr_mul_glv32_x2(pcr_load_affine(p_ws + i0, N), AgrWeight{w0.x, w0.y}, pcr_load_affine(p_ws + i1, N), AgrWeight{w1.x, w1.y}, r0, r1);
#endif
  const G1P id = proj_identity<Fp>();
  agr_store_point(w_ws + i0, W, proj_select((elig[g0] != 0) & !(flag[i0] & PCR_SKIP), r0, id));
  if (two) agr_store_point(w_ws + i1, W, proj_select((elig[g1] != 0) & !(flag[i1] & PCR_SKIP), r1, id));
}

// seg_of == nullptr: one segment (round 1).  Items: N pairs, then the V = S u virtual keys' identities
__global__ void __launch_bounds__(256) k_pcr_items(const uint32_t* gidx, const uint32_t* kid, const uint32_t* seg_of, size_t N, uint32_t u, uint32_t S,
                                                  int32_t* w_ws, size_t W, uint32_t* vkid, uint32_t* mkid) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, V = (size_t)S * u;
  if (i >= N + V) return;
  if (i < N) {
    vkid[i] = (seg_of ? seg_of[gidx[i]] : 0u) * u + kid[i];
    return;
  }
  const uint32_t v = (uint32_t)(i - N);
  agr_store_point(w_ws + i, W, proj_identity<Fp>());
  vkid[i] = v;
  mkid[v] = v % u;
}
