// pairing_check_rlc_plan.h -- host-side planning of the pairing-product checks over ragged groups by random linear combination
// (host_pairing_check_rlc.hip).  The segments, their bounds and the equation ranges that go to the exact call are
// aggregate_rlc_plan.h's (agr_pair_groups, agr_segments, agr_cut, agr_failed_ranges: an "equation" here is a "group" there, and a
// call has no signature items); what this call decides for itself is below.  Plain C++ over the standard library only, so that
// tests/hostsim/pairing_check_rlc_host.cpp compiles it for the CPU against a Python model.
#pragma once
#include "aggregate_rlc_plan.h"

// The default rule's cap on S.  The aggregate call's 16 (AGR_SMAX) was measured for THAT call;
// scripts/bench_pairing_check_rlc.py tried 16, 64 and 256 on the one-false-equation rows: 2^18 x 2 over two Q
// 24.6 / 20.4 / 18.3 ms (spreads 0.2 / 0.2 / 0.3), 2^14 x 2 10.3 / 8.7 / 8.7 ms (0.2 / 0.2 / 0.4), every other row within its
// spread -- a segment costs u Miller slots and one final exponentiation, which is little over two Q, while a failed segment
// sends a 1 / S share of the call to the exact call.  256 is the fastest or within the spread on every row.
static const size_t PCR_SMAX = 256;
// Two exact sub-calls are made one when fewer than this many pairs and equations lie between them.  The aggregate call's gap
// (2^16 items) stands for 10 ms per sub-call; blsbn254_pairing_check_batch has latency forms, so a small sub-call costs less:
// measured 4.25 ms for 2^10 x 2 against 64.1 ms for 2^18 x 2 (0.122 us per pair), so a small call's fixed cost is what the exact
// call takes for 34 783 pairs in a call that runs anyway: 2^15 (scripts/bench_pairing_check_rlc.py "merge_gap").
static const size_t PCR_MERGE_GAP = (size_t)1 << 15;

// Round 1 is taken when the G2 members repeat: u distinct encodings among the N pairs, each a table of its own (no table is
// appended: the call has no signature pair).  N == 0 (every equation empty) is the exact call's too: nothing to combine.
static inline bool pcr_round1(size_t N, size_t u, size_t max_keys) { return N != 0 && u * 2 <= N && u <= max_keys; }
