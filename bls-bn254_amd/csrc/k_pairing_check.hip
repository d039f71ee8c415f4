// k_pairing_check.hip -- pairing-product equations over ragged groups of pairs (multi_miller_loop(..).final_exponentiation()
// == Gt::identity, pairings.rs:706-713 with :698-704): the per-pair validity fold and the segmented product of the pairs'
// Miller values.  The Miller loops and the final exponentiation are the existing kernels; host side in host_pairing_check.hip.
#include "lane_ops.h"
#include "kernels.h"
using namespace bn;

// ok[i] = FLAG_SIG_OK | FLAG_PK_OK when P_i decodes and is on the curve (the identity allowed) and Q_i decodes, is on the curve
// and is the identity or lies in the r-torsion, else 0: the byte the final exponentiation's mode 0 expects in `flags` and
// `sub_ok` once the segmented product has ANDed it over an equation.  The torsion test runs only for a valid, non-identity Q
// (lane_g2_check would reject the identity), so a wave of identity / invalid members skips it.
BN_KERNEL k_pair_ok(const uint8_t* g1, const uint8_t* g2, size_t n, uint8_t* ok) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bool ok1, ok2;
  const G1A p = g1_decode(g1 + 64 * i, ok1);
  const G2A q = g2_decode(g2 + 128 * i, ok2);
  const bool p_ok = ok1 && g1_on_curve(p);
  bool q_ok = ok2 && g2_on_curve(q);
  if (q_ok && !q.inf) q_ok = g2_torsion_free(q);
  ok[i] = (p_ok && q_ok) ? (uint8_t)(FLAG_SIG_OK | FLAG_PK_OK) : (uint8_t)0;
}

// One lane per chunk: out[c] = product of the values chunk_start[c] .. + chunk_len[c] of in_ws (limb-major Fp12), ok_out[c] =
// AND of their ok bytes.  An empty chunk (an empty equation) gives Fp12::ONE with ok = FLAG_SIG_OK | FLAG_PK_OK.
// ok_in == nullptr: no flags (the Miller-value path; ok_out is not written).
// carry != 0: chunk 0 continues the product of an equation begun by an earlier launch, whose running value and flag are
// already at out[0] / ok_out[0]: the chunk's values are multiplied into it.
// The running product lives in the lane's own output column, not in registers: each step is one product of two loaded values
// (k_fp12_mul_pairs' shape, which fits the registers), 1.3 KB of traffic against ~18 K multiply-adds.  Both columns are read
// with buffer addressing (tower.h Ws: wave-uniform base, the lane's index in the lane offset), so no per-limb 64-bit address
// is held in vector registers across the loop.  0 B of scratch (tests/test_pairing_check_kernels.py).
BN_KERNEL k_fp12_seg_prod(const int32_t* in_ws, size_t in_stride, const uint8_t* ok_in, const uint32_t* chunk_start, const uint32_t* chunk_len,
                          size_t m, int32_t* out_ws, size_t out_stride, uint8_t* ok_out, int carry) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= m) return;
  const uint32_t s0 = chunk_start[c], len = chunk_len[c];
  const bool cont = carry && c == 0;
  Ws acc = {out_ws, out_stride, (uint32_t)c * 4u, true};
  uint8_t ok = (uint8_t)(FLAG_SIG_OK | FLAG_PK_OK);
  uint32_t j = 0;
  if (cont) {
    if (ok_in) ok = ok_out[0];
  } else {
    Ws v = {const_cast<int32_t*>(in_ws), in_stride, s0 * 4u, true};
    fp12_store_limbs(acc, len ? fp12_load_limbs(v) : fp12_one());
    if (ok_in && len) ok = ok_in[s0];
    j = 1;
  }
#pragma unroll 1
  for (; j < len; ++j) {
    Ws v = {const_cast<int32_t*>(in_ws), in_stride, (s0 + j) * 4u, true};
    BN_MEM_FENCE;
    fp12_store_limbs(acc, fp12_mul(fp12_load_limbs(acc), fp12_load_limbs(v)));
    if (ok_in) ok &= ok_in[s0 + j];
  }
  if (ok_in) ok_out[c] = ok;
}
