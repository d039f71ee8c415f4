// threshold_checked_host.cpp -- the lane functions of csrc/threshold_checked.h (selection for the checked threshold combine over
// many groups) compiled for the host with -DBN_CHECK (every field operation asserts the lazy-limb interval discipline), for
// tests/test_threshold_checked_host.py: candidate bits, repeated ids, ranks and compacted slots, run lane by lane over ONE
// launch [lo, lo + m) of the call's shares as the kernels of k_threshold_checked.hip index them.  TEST TOOL ONLY.
#include "../../bls-bn254_amd/csrc/threshold_checked.h"
#include <cstring>

using namespace bn;

extern "C" {

// k_tc_scan: cand[i] / repeat[i] for the lanes of the launch (one byte each; the kernel packs the first by ballot and folds
// the second into the group's mark word)
void hs_tc_scan(const uint8_t* ids, const uint8_t* sigs, const uint32_t* goff, uint32_t ng, uint32_t lo, uint32_t m, uint8_t* cand, uint8_t* repeat) {
  for (uint32_t i = 0; i < m; ++i) {
    const uint32_t s = lo + i, g = th_find_group(goff, ng, s);
    cand[i] = tc_candidate(sigs + 64 * (size_t)s) ? 1 : 0;
    repeat[i] = tc_repeats(ids, goff[g], s) ? 1 : 0;
  }
}

// k_tc_select: marks[g] in / out (the short mark is added), rank[i] / used[i] for the lanes of the launch, the picked shares
// copied to their slots of c_ids / c_sigs
void hs_tc_select(const uint8_t* bits_a, const uint8_t* bits_b, const uint32_t* goff, const uint32_t* coff, uint32_t ng, uint32_t* marks, uint32_t lo, uint32_t m,
                  const uint8_t* ids, const uint8_t* sigs, uint8_t* c_ids, uint8_t* c_sigs, uint32_t* rank, uint8_t* used) {
  for (uint32_t i = 0; i < m; ++i) {
    const uint32_t s = lo + i, g = th_find_group(goff, ng, s);
    const uint32_t a = goff[g], t = coff[g + 1] - coff[g];
    const TcRank r = tc_rank(bits_a, bits_b, a, goff[g + 1], s);
    if (s == a && tc_short(r, t)) marks[g] |= TC_MARK_SHORT;
    const bool u = tc_pick(r, t, marks[g]);
    rank[i] = r.rank; used[i] = u ? 1 : 0;
    if (u) {
      const size_t slot = (size_t)coff[g] + r.rank;
      std::memcpy(c_ids + 32 * slot, ids + 32 * (size_t)s, 32);
      std::memcpy(c_sigs + 64 * slot, sigs + 64 * (size_t)s, 64);
    }
  }
}

}  // extern "C"
