// k_aggregate_batch.hip -- aggregate verify over ragged groups of (key, message) pairs: the signatures' slots of the H
// workspace, the two-pairs-per-lane Miller loop over lanes planned per group, and the fold of the per-pair and per-group
// flags into the byte the segmented product ANDs over a group.  Host side in host_aggregate_batch.hip.
// Same compile policy as k_miller_hpk2 (-DBN_FORCE_INLINE -DBN_LC_MAD) and the same LDS budget: 144 limbs per lane.
//
// Slots.  The H workspace holds N + G affine points (18 limbs each, stride N + G): slot j < N is H(msg_j) of the caller's
// pair j, slot N + g is group g's aggregate signature.  A lane's descriptor names one or two slots of ONE group;
// AGB_NO_SLOT marks the missing half of a group with an odd number of pairs (its signature's pair counted).
#include "lane_ops.h"
#include "kernels.h"
using namespace bn;

// Group g's signature (64 bytes) -> slot n_pairs + g; sig_ok[g] = decodes, not the identity, on the curve.  A bad signature is
// replaced by the generator (uniform arithmetic in the Miller loop); its flag fails the group.  k_g1_to_ws over n_groups lanes.
BN_KERNEL k_agb_place_sigs(const uint8_t* sigs, size_t n_groups, int32_t* h_ws, size_t n_pairs, size_t h_stride, uint8_t* sig_ok) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups) return;
  bool okd;
  const G1A p = g1_decode(sigs + 64 * g, okd);
  const bool good = okd & !p.inf & g1_on_curve(p);
  G1A gp; gp.x = fp_one(); gp.y = fp_norm(fp_add(fp_one(), fp_one()));
  const size_t slot = n_pairs + g;
  store_fp(h_ws + slot, h_stride, fp_select(good, p.x, gp.x)); store_fp(h_ws + 9 * h_stride + slot, h_stride, fp_select(good, p.y, gp.y));
  sig_ok[g] = good ? 1 : 0;
}

// m lanes; lane i takes the slots slot_a[i] (always present) and slot_b[i] (or AGB_NO_SLOT).  A slot below n_pairs pairs its H
// point with the caller's key pks[128 slot]; a signature's slot pairs with -G2gen, taken from the constants: never read from
// memory, never validated.  q_ws: 72 x m limbs (stride m, written here), f_ws: 108 x f_stride,
// flags[slot] (caller's pairs only) = 1 when the key decodes, is not the identity and is on the curve.
// The loop body is k_miller_hpk2's: miller_loop_2var_ws, a one-slot lane masked by `live` as that kernel's padding half.
BN_KERNEL k_miller_hpk2r(const int32_t* h_ws, size_t h_stride, const uint8_t* pks, size_t n_pairs, const uint32_t* slot_a, const uint32_t* slot_b,
                         size_t m, int32_t* q_ws, int32_t* f_ws, size_t f_stride, uint8_t* flags) {
  __shared__ int32_t lds[144 * 256];             // each lane touches only its own column: no barrier needed
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const Ws hh = {lds, 256, threadIdx.x * 4u, false};
  const Ws park = ws_at(hh, 36), lpark = ws_at(hh, 90);
  const Ws qw = {q_ws, m, i * 4u, true};
  const uint32_t first = slot_a[i];
  bool live[2];
  for (int k = 0; k < 2; ++k) {
    const uint32_t s = k ? slot_b[i] : first;
    const bool present = s != AGB_NO_SLOT;
    const uint32_t src = present ? s : first;                      // missing half: re-read the lane's first slot, masked out below
    const bool is_sig = src >= n_pairs;
    bool okp;
    // a signature's half decodes key 0 and discards it (uniform control flow; little beside the loop).  Key 0 exists: the host
    // returns before any launch when n_pairs == 0 (blsbn254_aggregate_verify_batch, "every group is empty")
    G2A pk = g2_decode(pks + 128 * (size_t)(is_sig ? 0 : src), okp);
    const bool pk_ok = okp & !pk.inf & g2_on_curve(pk);
    const bool use = pk_ok & !is_sig;
    const Fp2 gy = fp2_const(bnc::G2_GEN_Y);
    pk.x = fp2_select(use, pk.x, fp2_const(bnc::G2_GEN_X)); pk.y = fp2_select(use, pk.y, fp2_select(is_sig, fp2_neg(gy), gy));
    fp2_store_mem(ws_at(qw, 36 * k), fp2_norm(pk.x)); fp2_store_mem(ws_at(qw, 36 * k + 18), fp2_norm(pk.y));
    const Ws hw = {const_cast<int32_t*>(h_ws), h_stride, src * 4u, true};
    // a missing half evaluates its (masked, constant 1) line at y = 1, so that it multiplies f by exactly 1
    fp_store_mem(ws_at(hh, 18 * k), fp_load_mem(hw)); fp_store_mem(ws_at(hh, 18 * k + 9), fp_select(present, fp_load_mem(ws_at(hw, 9)), fp_one()));
    if (present & !is_sig) flags[src] = pk_ok ? 1 : 0;
    live[k] = present;            // an invalid key still runs on the generator (uniform arithmetic); its flag fails its group
  }
  BN_MEM_FENCE;
  fp12_store_limbs(Ws{f_ws, f_stride, i * 4u, true}, miller_loop_2var_ws(hh, qw, park, lpark, live[0], live[1]));
}

// ok[i] for lane i of a launch = FLAG_SIG_OK | FLAG_PK_OK when every slot of the lane is good, else 0 -- the byte
// k_fp12_seg_prod ANDs over a group's lanes and the final exponentiation's mode 0 expects.  A caller's pair is good when its
// key passed the curve checks of the Miller kernel (flags) and the r-torsion test (sub_ok); a signature's slot carries its
// group's two conditions: the signature's flag, and the group has at least one pair (goff: the groups' pair offsets, rebased).
// Every group has exactly one signature slot, so each condition enters each group's AND once.
__global__ void __launch_bounds__(256) k_agb_fold(const uint32_t* slot_a, const uint32_t* slot_b, size_t m, size_t n_pairs, const uint8_t* flags,
                                                  const uint8_t* sub_ok, const uint8_t* sig_ok, const uint32_t* goff, uint8_t* ok) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  bool good = true;
  for (int k = 0; k < 2; ++k) {
    const uint32_t s = k ? slot_b[i] : slot_a[i];
    if (s == AGB_NO_SLOT) continue;
    if (s < n_pairs) good &= (flags[s] & sub_ok[s] & 1) != 0;
    else { const uint32_t g = s - (uint32_t)n_pairs; good &= sig_ok[g] == 1 && goff[g + 1] > goff[g]; }
  }
  ok[i] = good ? (uint8_t)(FLAG_SIG_OK | FLAG_PK_OK) : (uint8_t)0;
}
