// launch_forms.h -- which device form runs at which size, stated ONCE: the settings (LaunchForms, the context's `forms`), their
// environment overrides, and one pure function per decision the host units make with them.  The forms: one WAVE per element
// (wide.h), a quad of lanes per element (tri.h / quad.h: "tri", three of the four lanes carry an Fp12 value), one lane per
// element, and -- the table-only Miller loop over raw tables alone -- two pairs per lane.  All forms of a kernel give the same
// values; the rule only chooses the fastest.  The Miller loop of a pipeline and the final exponentiation behind it agree on the
// limits because both ask here.  Plain C++ over the standard library only (no HIP, no context), so that
// tests/hostsim/launch_forms_host.cpp compiles it for the CPU against a Python model.
#pragma once
#include <cstddef>
#include <cstdlib>

struct LaunchForms {
  size_t lanes_per_round = 65536;    // CUs x 256: the lanes resident at one wave per SIMD (the big kernels' occupancy)
  bool wide = true;                  // the wave-per-element kernels (BLSBN254_WIDE_FE=0: off) ...
  size_t wide_max = 2048;            // ... for launches of at most this many elements (BLSBN254_WIDE_FE_MAX): two rounds of a wave per tuple
                                     // cost what the quad kernels cost for anything up to 16384 (r03: 4096 wide = 7.8 ms, 4100 on quads = 5.6 ms)
  size_t tri_max = 16384;            // launches of up to lanes_per_round / 4 elements run a quad of lanes per element: one round of waves
                                     // (BLSBN254_TRI_MAX, 0 = off)
  bool tri_miller = true, tri_fe = true;   // BLSBN254_TRI_MILLER=0 / BLSBN254_TRI_FE=0: keep one of the two on the lane-per-element kernels (A/B runs)
  bool split_easy = true;            // BLSBN254_SPLIT_EASY=0: the one-launch easy part at every size
  bool quad_prep = true;             // per-key preparation with four lanes per key while that fits one round of waves (BLSBN254_QUAD_PREP=0: off)
};

// The settings of a device with `compute_units` CUs under the environment `get` reads (std::getenv, or a test's table).  Switches
// are atoi(e) != 0; the two limits are taken in 0 .. 1 << 20 and ignored outside; BLSBN254_TRI_MAX overrides the derived limit.
static inline LaunchForms forms_from_env(const char* (*get)(const char*), int compute_units) {
  LaunchForms F;
  const auto flag = [&](const char* name, bool& v) { if (const char* e = get(name)) v = std::atoi(e) != 0; };
  const auto limit = [&](const char* name, size_t& v) { if (const char* e = get(name)) { long x = std::atol(e); if (x >= 0 && x <= (1 << 20)) v = (size_t)x; } };
  F.lanes_per_round = (size_t)compute_units * 256;
  F.tri_max = F.lanes_per_round / 4;        // four lanes per element: one round of waves
  flag("BLSBN254_WIDE_FE", F.wide);
  flag("BLSBN254_QUAD_PREP", F.quad_prep);
  flag("BLSBN254_SPLIT_EASY", F.split_easy);
  flag("BLSBN254_TRI_MILLER", F.tri_miller);
  flag("BLSBN254_TRI_FE", F.tri_fe);
  limit("BLSBN254_TRI_MAX", F.tri_max);
  limit("BLSBN254_WIDE_FE_MAX", F.wide_max);
  return F;
}

enum class Form { WIDE, TRI, LANE };

// The hard part of the final exponentiation over n values.  Few: the lane-per-tuple kernels would be the latency of one lane's
// chain (4.5 ms for any n <= 65536), so one WAVE per tuple (k_fe_wide.hip): ~0.6 ms per round of CUs x 16 tuples.  Between that
// limit and a quarter of a round of lanes: a quad per tuple (k_tri.hip) -- one lane's whole chain would cost 5.4 ms however few
// tuples there are.  Beyond: t^x three times, one lane per tuple.
static inline Form fe_hard_form(const LaunchForms& F, size_t n) {
  if (F.wide && n <= F.wide_max) return Form::WIDE;
  if (F.tri_fe && n <= F.tri_max) return Form::TRI;
  return Form::LANE;
}
// The easy part: from half a round of waves up, the ONE Fp inversion is shared by four tuples per lane (head / inv4 / tail,
// k_fe_easy.hip); below, one launch.
static inline bool fe_easy_split(const LaunchForms& F, size_t n) { return n >= F.lanes_per_round / 2 && F.split_easy; }

// The Miller loop over n pairs of VARIABLE points (miller_to_ws).  Few pairs: one wave per pair -- lane 0 runs the G2 point
// arithmetic, and that serial part makes the chain ~2 x a prepared one, hence half the wave limit.  Mid-size: a quad of lanes per
// pair (line steps four lanes per point, f three lanes per value).  Else one lane per pair.
static inline Form miller_form(const LaunchForms& F, size_t n) {
  if (F.wide && n <= F.wide_max / 2) return Form::WIDE;
  if (F.tri_miller && n <= F.tri_max) return Form::TRI;
  return Form::LANE;
}

// The TABLE-ONLY Miller loops (launch_miller_prepared over expanded pair tables; launch_miller_raw over raw line tables, per
// launch chunk), among the forms the call site admits: one wave per pair up to the wave limit (k_miller_wide.hip), a quad of
// lanes per pair up to tri_max (k_tri.hip), else a lane.
enum : unsigned { MR_WIDE = 1, MR_TRI = 2, MR_ONE = 4, MR_TWO = 8, MR_ALL = 15 };
static inline Form table_miller_form(const LaunchForms& F, size_t n, unsigned admitted = MR_ALL) {
  if ((admitted & MR_WIDE) && F.wide && n <= F.wide_max) return Form::WIDE;
  if ((admitted & MR_TRI) && F.tri_miller && n <= F.tri_max) return Form::TRI;
  return Form::LANE;
}
// ... and whether the whole launch of n pairs over raw tables runs TWO pairs per lane sharing f^2 (k_miller_hpk2p) instead: when
// neither small form takes it and one pair per lane does not either.  One pair per lane takes it while 2 n <= lanes_per_round
// (the launch is the latency of one wave: no shared f^2, the shorter chain), when two per lane is not admitted, and when
// n > chunk (the per-pair forms run chunk by chunk).
static inline bool raw_two_per_lane(const LaunchForms& F, size_t n, unsigned admitted, size_t chunk) {
  const bool one = (admitted & MR_ONE) && (n * 2 <= F.lanes_per_round || !(admitted & MR_TWO) || n > chunk);
  return table_miller_form(F, n, admitted) == Form::LANE && !one;
}

// G2Prepared::from for u keys: four lanes per key (k_keyprep_quad.hip, half the latency) while the 8 u lanes fit one round of
// waves, else one lane per key (k_keyprep.hip)
static inline bool prepare_on_quads(const LaunchForms& F, size_t u) { return F.quad_prep && 8 * u <= F.lanes_per_round; }

// A launch of n tuples is small enough that the prepared-key path wins whatever its keys: with line tables the Miller loop (and
// the final exponentiation) can run one WAVE per tuple or, up to tri_max, a quad per tuple instead of at the latency of one lane
// -- a launch of that size is bound by latency, not by the table work (16 384 distinct keys: ~2 ms of preparation against 4 ms
// saved).  per_tuple_fe: the launch also runs a final exponentiation per tuple, so the quad form only pays when that half is
// enabled too (the grouped aggregate verify runs ONE final exponentiation and passes false).
static inline bool small_for_prepared(const LaunchForms& F, size_t n, bool per_tuple_fe) {
  return (F.wide && n <= F.wide_max) || (F.tri_miller && (F.tri_fe || !per_tuple_fe) && n <= F.tri_max);
}
// blsbn254_aggregate_verify counts its keys (aggregate_verify_grouped) below 1024 pairs only when its n pairs, the signature's
// among them, fit the wave-per-pair form: the quad forms do not count here (a call between the two limits goes pair by pair
// without the de-duplication's read-back).
static inline bool grouped_whatever_keys(const LaunchForms& F, size_t n) { return F.wide && n <= F.wide_max; }
