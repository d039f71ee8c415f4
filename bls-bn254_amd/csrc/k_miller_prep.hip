// k_miller_prep.hip -- the verify Miller loop for PREPARED public keys: f = ML(sig, -G2gen) * ML(H(msg), pk) with both
// pairs' line coefficients taken from tables, i.e. multi_miller_loop(&[(&G1Affine, &G2Prepared)]) of the reference
// (pairings.rs:808-857) for two terms -- and since the first term's table (-G2gen) is the same for every tuple, the per-key
// table holds the nine coefficient products of each step's line PAIR, divided by the one that multiplies xs X (k_g2_expand;
// pairing.h line_pair_expand_unit), and the tuple's coordinate values are divided by xs X: that coefficient of the pair is 1.
// No point arithmetic, no running point: per loop digit one squaring of f, four coefficient evaluations and one product of f with the
// pair in twelve Fp2 products (three 3 x 2 products over Fp2[w] by evaluation at 0, inf, 1, -1; pairing.h ell_pair_unit), which
// yields twice the value: the loop's result carries 2^88, removed by the final exponentiation like the other subfield factors.
// Lanes run in key-sorted order (perm), so a wave reads one key's table at (mostly) one address.
// Same compile policy as the other Miller units (-DBN_FORCE_INLINE -DBN_LC_MAD).
#include "lane_ops.h"
#include "kernels.h"
using namespace bn;

// sorted position s -> tuple perm[s] with key id kid[perm[s]].  f_ws / flags are in SORTED order.  h_ws: H(msg) homogeneous, 27 x h_stride limbs.
// flags[s] = signature decodes, is not the identity, is on the curve, AND the key passed its checks (key_ok).
BN_KERNEL k_miller_prepared(const uint32_t* perm, const uint32_t* kid, const uint8_t* sigs, const int32_t* h_ws, size_t h_stride,
                            const int32_t* table, const uint8_t* key_ok, size_t n, int32_t* f_ws, uint8_t* flags) {
  __shared__ int32_t inv_lds[72 * 256];          // each lane touches only its own column: no barrier needed
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const uint32_t i = perm[s], k = kid[i];
  bool oks;
  G1A sig = g1_decode(sigs + 64 * (size_t)i, oks);
  const bool sig_ok = oks & !sig.inf & g1_on_curve(sig);
  G1A gp; gp.x = fp_one(); gp.y = fp_norm(fp_add(fp_one(), fp_one()));
  const Ws inv = {inv_lds, 256, threadIdx.x * 4u, false};
  const Ws hw = {const_cast<int32_t*>(h_ws), h_stride, i * 4u, true};
  const Fp xs = fp_norm(fp_select(sig_ok, sig.x, gp.x)), ys = fp_norm(fp_select(sig_ok, sig.y, gp.y));
  const Fp X = fp_load_mem(hw), Y = fp_load_mem(ws_at(hw, 9)), Z = fp_load_mem(ws_at(hw, 18));       // H(msg) = (X : Y : Z), from k_hash_to_g1 mode 3
  // the eight coordinate values scaled by (xs X)^-1, so that the pair's v-coefficient is 1; unit = 0 for H(msg) = identity (X = 0),
  // whose lane keeps scale 1 and the true coefficient 0 (pairing.h miller_unit_coords)
  bool inv_ok;
  const bool unit = miller_unit_coords(xs, ys, X, Y, Z, inv, inv_ok);
  BN_MEM_FENCE;
  const Ws kt = {const_cast<int32_t*>(table), 1, k * (uint32_t)(BN_NEG_G2_LINES * 162 * 4), true};
  fp12_store_limbs(Ws{f_ws, n, s * 4u, true}, miller_loop_prepared_unit(inv, kt, unit));
  flags[s] = (sig_ok && inv_ok && key_ok[k] != 0) ? 1 : 0;          // inv_ok: always, by the bound of the divstep recurrence; fails closed
}
