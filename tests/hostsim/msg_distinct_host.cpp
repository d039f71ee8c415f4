// msg_distinct_host.cpp -- the lane functions of csrc/msg_distinct.h (the distinct-message rule of the aggregate verify over
// groups: md_key, md_insert) compiled for the host with -DBN_CHECK and run lane by lane, in an order the caller names, over
// buffers of exactly the size the kernels are given.  As a shared object tests/test_msg_distinct_host.py compares every table and
// every dup byte with the Python model of tests/msg_distinct_support.py -- once as the library has it and once with
// -DMD_SLOT_HASH_ZERO, where every key starts at slot 0; as a stand-alone program (main below; built with the address and
// undefined-behaviour sanitizers) it runs the same functions against a brute-force comparison of the keys.
// TEST TOOL ONLY: the product has no CPU path.
#include "../../bls-bn254_amd/csrc/msg_distinct.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace bn;

extern "C" {

uint32_t hs_md_slots(uint32_t n) { return md_slots(n); }
void hs_md_p_limbs(int32_t* out) { for (int k = 0; k < NL; ++k) out[k] = bnc::P[k]; }
// 32 big-endian bytes (< p) -> the canonical Montgomery limbs a workspace holds for that value
int hs_md_fp_limbs(const uint8_t* be, int32_t* out) {
  bool ok;
  const Fp c = fp_canon(fp_from_be(be, ok));
  for (int k = 0; k < NL; ++k) out[k] = c.l[k];
  return ok ? 1 : 0;
}
// k_md_keys: pts limb-major with stride `stride` (18 or 27 rows), key 18 rows of n
void hs_md_keys(const int32_t* pts, size_t stride, uint32_t n, int form, int32_t* key) {
  for (uint32_t i = 0; i < n; ++i) md_key(pts + i, stride, form, key + i, n);
}
// key i as the 64 bytes x || y of the encodings
void hs_md_key_bytes(const int32_t* key, uint32_t n, uint32_t i, uint8_t* out) {
  Fp x, y;
  for (int k = 0; k < NL; ++k) { x.l[k] = key[(size_t)k * n + i]; y.l[k] = key[(size_t)(NL + k) * n + i]; }
  BN_TRK(set_trk(x, 0, 1, 0, 0.006, 1); set_trk(y, 0, 1, 0, 0.006, 1);)
  fp_to_be(out, x); fp_to_be(out + 32, y);
}
uint32_t hs_md_slot_hash(uint32_t g, const int32_t* key, uint32_t n, uint32_t i, uint32_t seed) { return md_slot_hash(g, key + i, n, seed); }
uint32_t hs_md_group_of(const uint32_t* goff, uint32_t G, uint32_t i) { return md_group_of(goff, G, i); }
// what the stage does behind the keys: the table (M = mask + 1 entries) and dup[] (G bytes) cleared, then k_md_insert's lanes in
// the order `order` names them (n entries, a permutation of 0 .. n - 1)
void hs_md_insert_all(uint32_t n, const uint32_t* goff, uint32_t G, const int32_t* key, const uint32_t* order, uint32_t* slots, uint32_t mask, uint32_t seed,
                      uint8_t* dup) {
  for (uint32_t s = 0; s <= mask; ++s) slots[s] = KC_EMPTY;
  for (uint32_t g = 0; g < G; ++g) dup[g] = 0;
  for (uint32_t j = 0; j < n; ++j) md_insert(order[j], n, goff, G, key, slots, mask, seed, dup);
}

}  // extern "C"

namespace {
int fails = 0;
void expect(bool ok, const char* what, size_t at) { if (!ok) { std::fprintf(stderr, "FAIL %s (%zu)\n", what, at); ++fails; } }

Fp small(uint32_t v) {                                   // the field element v, Montgomery
  Fp p = fp_zero();
  p.l[0] = (int32_t)(v & (uint32_t)MASK);
  BN_TRK(set_trk(p, 0, 1, 0, 0, 1e-60);)
  return fp_to_mont(p);
}
void put(std::vector<int32_t>& ws, size_t stride, size_t row, size_t i, const Fp& a, bool shifted) {
  Fp c = fp_canon(a);
  if (shifted) for (int k = 0; k < NL; ++k) c.l[k] += bnc::P[k];         // the same value in another limb pattern
  for (int k = 0; k < NL; ++k) ws[(row + (size_t)k) * stride + i] = c.l[k];
}
// dup[] by comparing every two keys of a group
std::vector<uint8_t> brute(const std::vector<int32_t>& key, uint32_t n, const std::vector<uint32_t>& goff) {
  const uint32_t G = (uint32_t)goff.size() - 1;
  std::vector<uint8_t> dup(G, 0);
  for (uint32_t g = 0; g < G; ++g)
    for (uint32_t a = goff[g]; a < goff[g + 1]; ++a)
      for (uint32_t b = a + 1; b < goff[g + 1]; ++b)
        if (md_key_equal(key.data() + a, key.data() + b, n)) dup[g] = 1;
  return dup;
}
}  // namespace

int main() {
  // 23 pairs: three in front of the first group, then groups of 0, 1, 2, 3, 0, 9 and 5 pairs; the point of pair i is the
  // small value v[i] (x = v, y = v + 1), so equal v = equal point
  const uint32_t n = 23;
  const std::vector<uint32_t> goff = {3, 3, 4, 6, 9, 9, 18, 23};
  const uint32_t G = (uint32_t)goff.size() - 1;
  const uint32_t v[n] = {7, 8, 9, /*g1*/ 7, /*g2*/ 5, 5, /*g3*/ 1, 2, 3, /*g5*/ 10, 11, 12, 13, 14, 15, 16, 17, 10, /*g6*/ 7, 20, 21, 22, 23};
  const std::vector<uint8_t> want = {0, 0, 1, 0, 0, 1, 0};
  std::vector<int32_t> aff(18 * (size_t)n), hom(27 * (size_t)n), ka(18 * (size_t)n), kh(18 * (size_t)n);
  for (uint32_t i = 0; i < n; ++i) {
    const Fp x = small(v[i]), y = small(v[i] + 1), z = small(1000 + 37 * i);
    put(aff, n, 0, i, x, i % 2 == 1); put(aff, n, 9, i, y, i % 3 == 1);
    put(hom, n, 0, i, fp_mul(x, z), i % 3 == 0); put(hom, n, 9, i, fp_mul(y, z), false); put(hom, n, 18, i, z, i % 2 == 0);
  }
  hs_md_keys(aff.data(), n, n, MD_AFFINE, ka.data());
  hs_md_keys(hom.data(), n, n, MD_HOMOGENEOUS, kh.data());
  expect(ka == kh, "the homogeneous form normalises to the affine keys", 0);
  expect(brute(ka, n, goff) == want, "the brute-force rule on the keys", 0);
  std::vector<uint32_t> order(n);
  for (uint32_t i = 0; i < n; ++i) order[i] = i;
  for (int round = 0; round < 6; ++round) {
    for (uint32_t M : {md_slots(n), 64u * md_slots(n)}) {
      std::vector<uint32_t> slots(M);
      std::vector<uint8_t> dup(G, 0xcc);
      hs_md_insert_all(n, goff.data(), G, ka.data(), order.data(), slots.data(), M - 1, 0x1234u + (uint32_t)round, dup.data());
      expect(dup == want, "dup[] of the table", (size_t)round);
      size_t taken = 0;
      for (uint32_t s = 0; s < M; ++s) taken += slots[s] != KC_EMPTY ? 1 : 0;
      expect(taken == n - 3 - 2, "one slot per distinct key of a group", (size_t)round);       // 20 pairs in groups, two of them repeats
    }
    std::next_permutation(order.begin(), order.end());
    std::rotate(order.begin(), order.begin() + 5, order.end());
  }
  // tables with fewer slots than keys: the probe wraps, ends after M slots and marks the group (fail closed) -- every group
  // that the full table marks stays marked
  for (uint32_t M : {2u, 4u}) {
    std::vector<uint32_t> slots(M);
    std::vector<uint8_t> dup(G, 0xcc);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    hs_md_insert_all(n, goff.data(), G, ka.data(), order.data(), slots.data(), M - 1, 99u, dup.data());
    for (uint32_t g = 0; g < G; ++g) expect(dup[g] <= 1 && dup[g] >= want[g], "fail closed never clears a repeat", g);
    expect(dup[0] == 0 && dup[4] == 0, "an empty group is never marked", M);
    expect(dup[5] == 1 && dup[6] == 1, "a group that finds no free slot is marked", M);
  }
  // every insertion order of a 4-pair group with a triple repeat
  {
    const uint32_t m = 4, w[m] = {4, 6, 4, 4};
    const std::vector<uint32_t> go = {0, 4};
    std::vector<int32_t> ws(18 * (size_t)m), key(18 * (size_t)m);
    for (uint32_t i = 0; i < m; ++i) { put(ws, m, 0, i, small(w[i]), i == 2); put(ws, m, 9, i, small(w[i] + 1), i == 3); }
    hs_md_keys(ws.data(), m, m, MD_AFFINE, key.data());
    std::vector<uint32_t> ord = {0, 1, 2, 3}, slots(md_slots(m));
    size_t count = 0;
    do {
      uint8_t dup = 0xcc;
      hs_md_insert_all(m, go.data(), 1, key.data(), ord.data(), slots.data(), md_slots(m) - 1, 5u, &dup);
      expect(dup == 1, "a triple repeat in every order", count);
      ++count;
    } while (std::next_permutation(ord.begin(), ord.end()));
    expect(count == 24, "24 orders", count);
  }
  if (fails) return 1;
  std::printf("msg_distinct_host ok\n");
  return 0;
}
