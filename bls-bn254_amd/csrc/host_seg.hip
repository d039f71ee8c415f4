// host_seg.hip -- what the calls over ragged groups share on the host side besides the planners (seg_plan.h) and the level
// loop (seg_run_levels, host_common.h): the staging of a segmented reduction's buffers and descriptors, and of a call's group
// offsets.  No kernels of its own; see host_common.h.
#include "host_common.h"

extern "C" {

int seg_stage(blsbn254_ctx* c, SegWs& w, size_t items_max, size_t limbs, bool flags) {
  for (int k = 0; k < 2; ++k) {
    HIPCHK(c, w.seg[k].reserve(items_max * limbs * 4));
    if (flags) HIPCHK(c, w.seg_ok[k].reserve(items_max));
  }
  TRY(upload(c, w.start, w.h_start.data(), 4 * w.h_start.size()));
  return upload(c, w.len, w.h_len.data(), 4 * w.h_len.size());
}

int stage_group_offsets(blsbn254_ctx* c, GroupOff& o, const uint64_t* off, size_t n_groups) {
  // the entry points reject such a call by name (CHECK_LANES); this guards the narrowing below where it happens
  if (off[n_groups] - off[0] > MAX_LANES) { c->last_error = "internal: group offsets span more than 2^23 elements"; return BLSBN254_E_HIP; }
  o.h.resize(n_groups + 1);
  for (size_t g = 0; g <= n_groups; ++g) o.h[g] = (uint32_t)(off[g] - off[0]);
  return upload(c, o.d, o.h.data(), 4 * (n_groups + 1));
}

}  // extern "C"
