// threshold_keycheck.h -- what ONE lane does in the check of dealt key shares against a group's Feldman commitments
// (k_threshold_keycheck.hip, host_threshold_deal.hip): one lane per SHARE,
//     [s_i] G2gen == sum_j [id_i^j] C_j
// The right-hand side is the key share k_g2_poly_eval left in the call's workspace (threshold_deal.h g2_horner_lane); the left
// one is a FIXED-BASE multiplication: s = sum_w d_w 2^(B w) in KC_WINDOWS digits of B = KC_WINDOW_BITS bits, so
//     [s] G2gen = sum_w tab[w][d_w],     tab[w][d] = [d 2^(B w)] G2gen,
// KC_WINDOWS - 1 complete additions and no doubling.  tab[w][0] is the identity (0 : 1 : 0), so a zero digit is one more
// complete addition and no lane branches on its digits; the table INDEX is the share's digit, so the check is not constant time.
//   kc_table_lane        lane w builds row w of the table: B w doublings of the generator constant, then 2^B - 2 additions
//   kc_share_words       a share's 32 big-endian bytes as little-endian words, ok = below r (zero is a share like any other)
//   kc_fixed_base_lane   the sum over the windows; entries are homogeneous (Proj<Fp2>), added with proj_add
//   kc_key_check_lane    proj_eq of that sum and the lane's key share: cross-multiplied, no inversion, the identity equal to itself
// B = 8: 32 windows of 256 entries, 31 additions per share, a table of 1.77 MB; B = 4: 64 x 16 entries, 63 additions, 221 KB.
// Either is larger than LDS and is read through L2; the 8-bit table halves the check kernel's time and is the one built.
// Table layout: entry e = w 2^B + d holds its 54 canonical limbs (x.c0, x.c1, y.c0, y.c1, z.c0, z.c1) CONTIGUOUSLY, 216 bytes
// at tab + 54 e.  The lanes of a wave read different entries, so the limb-major layout of the workspaces (a limb of all
// elements side by side) would make every one of an entry's 54 dwords a scattered access; here a lane's entry is 27 aligned
// 8-byte loads out of two or three 128-byte lines.
// tests/hostsim/threshold_keycheck_host.cpp runs the same functions on the host with -DBN_CHECK (interval discipline) against
// the oracle.  They are not a CPU fallback: nothing in the product's host path calls them.
#pragma once
#include "threshold_deal.h"

#ifndef BN_KC_WINDOW_BITS
#define BN_KC_WINDOW_BITS 8              // THE window width: 8 (measured) or 4; a measurement build passes -DBN_KC_WINDOW_BITS=4
#endif

namespace bn {

constexpr int KC_WINDOW_BITS = BN_KC_WINDOW_BITS;
constexpr int KC_WINDOWS = 256 / KC_WINDOW_BITS;                 // windows over the 256 bits of a share's bytes
constexpr int KC_DIGITS = 1 << KC_WINDOW_BITS;                   // entries per window
constexpr int KC_ENTRY_LIMBS = 54;                               // a homogeneous G2 point
constexpr size_t KC_TABLE_LIMBS = (size_t)KC_WINDOWS * KC_DIGITS * KC_ENTRY_LIMBS;
static_assert(32 % KC_WINDOW_BITS == 0 && KC_WINDOW_BITS <= 8, "a window never straddles a word");

struct alignas(8) KcPair { int32_t a, b; };                      // an entry is read and written as 27 of these

BN_INL void kc_store_entry(int32_t* tab, uint32_t e, const G2P& p) {
  const Fp c[6] = {fp_canon(p.x.c0), fp_canon(p.x.c1), fp_canon(p.y.c0), fp_canon(p.y.c1), fp_canon(p.z.c0), fp_canon(p.z.c1)};
  int32_t l[KC_ENTRY_LIMBS];
  BN_UNROLL for (int f = 0; f < 6; ++f) BN_UNROLL for (int k = 0; k < NL; ++k) l[NL * f + k] = c[f].l[k];
  KcPair* q = reinterpret_cast<KcPair*>(tab) + (size_t)(KC_ENTRY_LIMBS / 2) * e;
  BN_UNROLL for (int k = 0; k < KC_ENTRY_LIMBS / 2; ++k) q[k] = {l[2 * k], l[2 * k + 1]};
}
// e is the lane's own; tab is the same for every lane (a kernel argument), so the address is one base plus a 32-bit lane offset
BN_INL G2P kc_load_entry(const int32_t* tab, uint32_t e) {
  const KcPair* q = reinterpret_cast<const KcPair*>(tab) + (size_t)(KC_ENTRY_LIMBS / 2) * e;
  int32_t l[KC_ENTRY_LIMBS];
  BN_UNROLL for (int k = 0; k < KC_ENTRY_LIMBS / 2; ++k) { const KcPair v = q[k]; l[2 * k] = v.a; l[2 * k + 1] = v.b; }
  Fp c[6];
  BN_UNROLL for (int f = 0; f < 6; ++f) {
    BN_UNROLL for (int k = 0; k < NL; ++k) c[f].l[k] = l[NL * f + k];
    BN_TRK(set_trk(c[f], 0, 1, 0, 0.006, 1);)
  }
  return {{c[0], c[1]}, {c[2], c[3]}, {c[4], c[5]}};
}

// row w of the table (w < KC_WINDOWS): entries w 2^B .. w 2^B + 2^B - 1
BN_FUNC void kc_table_lane(int32_t* tab, uint32_t w) {
  BN_CTX;
  G2A g; g.x = fp2_const(bnc::G2_GEN_X); g.y = fp2_const(bnc::G2_GEN_Y); g.inf = false;
  G2P p = proj_from_affine(g);
#pragma unroll 1
  for (uint32_t i = 0; i < (uint32_t)KC_WINDOW_BITS * w; ++i) p = proj_dbl(p);
  const uint32_t e0 = w * (uint32_t)KC_DIGITS;
  kc_store_entry(tab, e0, proj_identity<Fp2>());
  kc_store_entry(tab, e0 + 1, p);
  G2P q = p;
#pragma unroll 1
  for (uint32_t d = 2; d < (uint32_t)KC_DIGITS; ++d) { q = proj_add(q, p); kc_store_entry(tab, e0 + d, q); }
}

// the share's bytes as the words the windows are cut from; ok = the value is below r (fr_from_be's flag: zero passes)
BN_INL void kc_share_words(const uint8_t* share, uint32_t k[8], bool& ok) {
  (void)fr_from_be(share, ok);
  BN_UNROLL for (int j = 0; j < 8; ++j) k[j] = load_be32(share + 4 * (7 - j));
}

// sum_w tab[w][digit w of k]: [k] G2gen for every 256-bit k (for k >= r too: the caller discards that lane through ok)
BN_FUNC G2P kc_fixed_base_lane(const int32_t* tab, const uint32_t* k) {
  BN_CTX;
  constexpr int PER_WORD = 32 / KC_WINDOW_BITS;
  G2P acc = kc_load_entry(tab, k[0] & (uint32_t)(KC_DIGITS - 1));
#pragma unroll 1
  for (uint32_t w = 1; w < (uint32_t)KC_WINDOWS; ++w) {
    const uint32_t j = w / PER_WORD;
    uint32_t v = 0;
    BN_UNROLL for (uint32_t q = 0; q < 8; ++q) v = q == j ? k[q] : v;        // w is uniform: selects, not an indexed array
    const uint32_t d = (v >> ((w % PER_WORD) * KC_WINDOW_BITS)) & (uint32_t)(KC_DIGITS - 1);
    acc = proj_add(acc, kc_load_entry(tab, w * (uint32_t)KC_DIGITS + d));
  }
  return acc;
}

// the share with the words k (ok: below r) against its key share: the same group element, the identity included
BN_FUNC bool kc_key_check_lane(const int32_t* tab, const uint32_t* k, bool ok, const G2P& key) {
  return ok & proj_eq(kc_fixed_base_lane(tab, k), key);
}

}  // namespace bn
