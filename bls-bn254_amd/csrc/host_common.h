// host_common.h -- shared by the host-side translation units (host*.hip): device buffers, ONE workspace struct per pipeline
// holding its buffers, the host copies its uploads read, its settings and its counters (MsmWs ... MdWs; the verify path: FeWs,
// KeyDedupWs, PrepWs, KeyStore, VerifyQueue; the batch verification by random linear combination: KeySumWs, Rlc2Ws, RlcWs), the
// context that holds one of each beside the staging buffers all pipelines share, the launch helper and the internal helpers one
// pipeline borrows from another.  The host-only rules live in plan headers without HIP: launch_forms.h (which device form runs at
// which size: the context's `forms`, asked by every launcher), rlc_plan.h, seg_plan.h and the keyset / aggregate plans.  Nothing
// here is exported (BNH = hidden visibility); the C ABI is include/blsbn254.h.  There is no CPU fallback anywhere on the host
// side: every entry point launches kernels or fails.
#pragma once
#include <hip/hip_runtime.h>
#include <sys/random.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "keccak.h"      // (with sha256.h) host-side use: pre-hashing an oversize DST only (RFC 9380 5.3.3); the expander ids
#include "lane_ops.h"    // flag constants
#include "kernels.h"
#include "key_cache.h"   // the store of prepared keys: its state words and kernels
#include "msg_distinct.h" // the distinct-message rule of the aggregate verify over groups: its forms, table size and kernels
#include "seg_plan.h"    // SegLevel, SegLaunch, the planners of the segmented reductions
#include "keyset_agg_plan.h"   // KaRepack, the argument walk of the checked aggregation over a key set
#include "keyset_merge_plan.h" // KmRepack, the argument walk of the checked merge over a key set
#include "keyset_weight_plan.h" // KwRepack, the column-total check and the quorum rule of the weights over a key set
#include "keyset_committee_plan.h" // KcTable, KcPlan: the committee tables of a key set and the plan of a call over them
#include "keyset_committee_agg_plan.h" // KcaRepack, the argument walk of the checked aggregation per committee of a key set
#include "keyset_committee_merge_plan.h" // KcmRepack, the argument walk of the checked merge per committee of a key set
#include "keyset_rlc_plan.h"   // KsrPlan: classes, chunks and runs of the key-set verify by random linear combination
#include "aggregate_rlc_plan.h" // the segments and exact ranges of the aggregate verify over groups by random linear combination
#include "pairing_check_rlc_plan.h" // the round-1 rule, the cap on S and the merge gap of the pairing-product checks by random linear combination
#include "launch_forms.h"      // LaunchForms and THE rule of every launcher: which device form runs at which size
#include "rlc_plan.h"          // the chunk size, the bounds and the key round's back-off of the batch verification by random linear combination
#include "../../include/blsbn254.h"

using namespace bn;

#define BNH __attribute__((visibility("hidden")))     // nothing of the host side is exported but the C ABI

// ------------------------------------------------------------------ host side
// A device allocation that grows on demand and frees itself: a DevBuf member of the context (or of a prepared-key table) needs
// no entry in any release list.  Not copyable.  Whoever destroys the owner first makes sure no stream still runs work on it.
struct BNH DevBuf {
  void* p = nullptr; size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
};
// multi-scalar multiplication (host_msm.hip, k_msm_bucket.hip): point rows, bucket entries, sorted entries, bucket counts and ends,
// the levels' partial sums (ping-pong), the bucket sums, the window segments, the device-side counters; reserved for the largest call
// blsbn254_msm_stats, in its order: bucket-path calls, small-n calls, bucket entries accumulated, level-0 chunks summed
struct BNH MsmWs { DevBuf pts, key, val, sorted, hist, end, part[2], bsum, seg, dstat; uint64_t stat[4] = {0, 0, 0, 0}; };
// A segmented reduction over ragged groups (seg_plan.h, seg_stage / seg_run_levels below): the levels between the first and the
// last (ping-pong) with their flags, and the run descriptors of every level of every launch of a call, on the device and as the
// host copies they are uploaded from.  The rule for every host copy an upload reads (these, GroupOff::h, the h_* / s_* vectors
// below): it is a member of the context, so it outlives the asynchronous copy, because every entry point ends synchronised.
// One instance per user: the host copies live for a whole call, and one call may run two reductions.
struct BNH SegWs {
  DevBuf seg[2], seg_ok[2], start, len;
  std::vector<uint32_t> h_start, h_len;
};
// a call's group offsets rebased to 0, 32-bit: on the device and the host copy they are uploaded from (stage_group_offsets)
struct BNH GroupOff { DevBuf d; std::vector<uint32_t> h; };
// pairing-product equations (host_pairing_check.hip, k_pairing_check.hip): per-equation products (limb-major, stride n_eq) and
// validity, per-pair validity of a launch, the product levels
struct BNH PcWs { DevBuf prod, ok, pair_ok; SegWs seg; };
// threshold combine over groups (host_threshold_batch.hip, k_threshold_batch.hip): the groups' offsets, per-share group words,
// the products, the levels of the group sums, the sums, the per-group marks, the encodings and statuses
// blsbn254_threshold_batch_stats: groups served by the lane-per-share kernels, groups handed to the single-group pipeline, launches
struct BNH ThbWs { GroupOff goff; DevBuf gid, pts, gsum, gstat, out, st; SegWs seg; uint64_t stat[3] = {0, 0, 0}; };
// aggregate verify over groups (host_aggregate_batch.hip, k_aggregate_batch.hip): the lanes' slot descriptors (device buffers and
// the host copies they are uploaded from), the groups' pair offsets, the signatures' flags.  The products and their levels are PcWs's.
struct BNH AgbWs {
  DevBuf slot_a, slot_b, sig_ok;
  GroupOff goff;
  std::vector<uint32_t> h_slot_a, h_slot_b;
  uint64_t stat[4] = {0, 0, 0, 0};   // groups served, lanes run by the two-pair kernel, calls served by the small forms, launches
};
// key shares and their public keys over groups (host_threshold_deal.hip, k_threshold_deal.hip): the staged coefficients /
// commitments and ids, the decoded coefficients (9 x T limbs) / loaded commitments (54 x T limbs) with their validity bytes, the
// shares before their encoding (9 x N / 54 x N limbs), the groups' id and coefficient offsets, the per-group marks and statuses,
// the public key shares in wire format; the host copies the per-share messages are uploaded from.  The check of dealt key shares
// (k_threshold_keycheck.hip): the staged shares and the byte per share its lanes leave
struct BNH TdlWs {
  DevBuf coef, ids, cf_ws, c_ws, c_ok, c_sub, r_ws, gstat, st, pks, shares, share_ok;
  GroupOff goff, coff;
  std::vector<uint8_t> h_msgs;
  std::vector<uint64_t> h_moff;
  uint64_t stat[4] = {0, 0, 0, 0};   // launches of the G2 evaluation, shares evaluated in G2, shares evaluated in Fr, bits of the last G2 launch
};
// checked threshold combine over groups (host_threshold_checked.hip, k_threshold_checked.hip): the staged ids and partial
// signatures, the candidate and used bitmaps over the call's shares, the compacted ids / partial signatures (t_g slots per group),
// the groups' id and coefficient offsets, marks and statuses, the groups' keys C_0 and their verification bits; the host copies
// the marks / bits are downloaded to, and the repacked arrays and results of the fallback's sub-call.  The commitments are
// staged and checked in TdlWs's buffers (td_stage_commitments).
struct BNH TcWs {
  DevBuf ids, sigs, cand, used, c_ids, c_sigs, gstat, st, keys, gbits;
  GroupOff goff, coff;
  std::vector<uint32_t> h_gstat;
  std::vector<uint8_t> h_gbits, s_commit, s_ids, s_sigs, s_msgs, s_out, s_used;
  std::vector<uint64_t> s_coff, s_goff, s_moff;
  std::vector<size_t> fail;
  uint64_t stat[4] = {0, 0, 0, 0};   // groups settled by the optimistic attempt, groups sent to the per-share fallback, shares verified individually, short groups
};
// sums over a registered key set selected by bitmaps (host_keyset.hip, k_keyset.hip): the call's rows, the groups' flip / ok bytes,
// the word-major partials of a launch and of its reduction passes (ping-pong); the host copy the flip bytes are downloaded to
// blsbn254_keyset_stats: groups served, groups summed through the complement, launches of the word kernel, key sets created
struct BNH KsetWs { DevBuf sel, flip, ok, part[2]; std::vector<uint8_t> h_flip; uint64_t stat[4] = {0, 0, 0, 0}; };
// What the four checked calls over a registered key set hold alike (host_keyset_checked.hip; aggregation and merge, full-width and
// per committee: DESIGN.md 6i, 6j, 6o, 6p, 6q).  An "entry" is a signature of the aggregation forms, a contribution of the merge
// forms.  On the device: the entries' signatures as 64-byte encodings (sigs) and, wire-format forms, as the 32 bytes uploaded
// (wire); the candidate bitmap over the entries and (merge forms) the used one; the signatures as points (27 x N limbs), the
// groups' sums with the levels between them (seg), the sums' encodings (out: 64 bytes, wout: 32 bytes, wire-format forms), the
// groups' rows as they leave (orows), the bits of the groups' equation (gbits), the entry offsets (goff); for the fallback the
// bits of the per-entry verification (vbits).  Host side: what an attempt downloads (h_*), the groups that go to the fallback
// (fail), the sub-call's messages (s_msgs / s_moff: one per group for the equation; s_emsgs / s_emoff: one per entry for the
// per-entry verification) and results (s_out, s_rows); the row offsets g * row_bytes the full-width forms address their rows by.
struct BNH CkWs {
  DevBuf sigs, wire, cand, used, pts, gsum, out, wout, orows, gbits, vbits;
  GroupOff goff;
  SegWs seg;
  std::vector<uint8_t> h_gbits, h_used, h_cand, s_msgs, s_emsgs, s_out, s_rows;
  std::vector<uint64_t> s_moff, s_emoff, even_off;
  std::vector<size_t> fail;
  // each form's ..._stats: groups settled by the optimistic attempt, groups sent to the per-entry fallback, entries verified individually, short groups
  uint64_t stat[4] = {0, 0, 0, 0};
};
// ... and each form's own (KcaWs, KcmWs: behind KcWs).  Aggregation (host_keyset_agg.hip): the staged indices, the keys the
// fallback gathers, the sub-call (keyset_agg_plan.h KaRepack) and its signatures
struct BNH KaggWs : CkWs { DevBuf idx, pks; KaRepack sub; std::vector<uint8_t> s_sigs; };
// the merge forms (ck_select, ck_verify_contributions): the contributions' rows as staged, the signature test and the selection's
// byte per contribution; merge (host_keyset_merge.hip): the sub-call (keyset_merge_plan.h KmRepack)
struct BNH KmStage : CkWs { DevBuf rows, sig_ok, flags; };
struct BNH KmWs : KmStage { KmRepack sub; };
// stake weights by bitmap and the verify with a quorum over a registered key set (host_keyset_weight.hip, k_keyset_weight.hip):
// the groups' weights of a call; host side the key-major table a blsbn254_keyset_set_weights uploads, the row that selects every
// key (the totals are its weights), the groups that reach quorum and their sub-call (keyset_weight_plan.h KwRepack) with its bits
struct BNH KwWs {
  DevBuf out;
  KwRepack sub;
  std::vector<uint64_t> h_tab;
  std::vector<uint8_t> h_ones, h_bits;
  std::vector<size_t> reach;
  uint64_t stat[4] = {0, 0, 0, 0};   // groups weighed, groups below quorum (not paired), launches of k_ks_weight for them, weight tables set
};
// committees over a registered key set (host_keyset_committee.hip, k_keyset_committee.hip): the call's rows; per sorted group its
// committee, row offset, partial base and caller's group; the items; the flip / ok bytes; the group-major partials of a launch
// with their (constant 1) flags; the reduced sums by sorted position with theirs; the levels between them; the committee of every
// committee word of a table being set; the weights of a call.  Host side: the plan (its vectors are what the uploads read), the
// flip bytes a call downloads, and the rows, offsets and committees of the call that sums a new table's totals.
struct BNH KcWs {
  DevBuf sel, scom, srow, spbase, order, items, flip, ok, part, part_ok, u, u_ok, wcom, wout;
  SegWs seg;
  KcPlan plan;
  std::vector<uint8_t> h_flip, h_ones;
  std::vector<uint64_t> h_off;
  std::vector<uint32_t> h_com;
  uint64_t stat[4] = {0, 0, 0, 0};   // groups served, groups summed through the complement, launches of the word kernel, committee tables set
};
// aggregation per committee (host_keyset_committee_agg.hip; the key sums run in KcWs): positions in place of indices; the
// groups' committees, the prefix of their row words and the byte offsets of their rows (device buffers and the host copies they
// are uploaded from); for the fallback the registry indices the positions resolve to and the gathered keys; the sub-call
// (keyset_committee_agg_plan.h KcaRepack) and its signatures
struct BNH KcaWs : CkWs {
  DevBuf com, pos, pks, ridx, wpre, roff;
  KcaRepack sub;
  std::vector<uint64_t> h_wpre, h_roff;
  std::vector<uint8_t> s_sigs;
};
// merge per committee (host_keyset_committee_merge.hip): ragged rows (the merged rows in orows at the caller's sel_off
// positions); the groups' committees and the byte offsets of their contribution rows and of their merged rows (device buffers
// and the host copies they are uploaded from); for the fallback the committee and the row offset of every contribution; the
// sub-call (keyset_committee_merge_plan.h KcmRepack)
struct BNH KcmWs : KmStage {
  DevBuf com, rbase, roff;
  KcmRepack sub;
  std::vector<uint64_t> h_rbase, h_roff, h_coff;
  std::vector<uint32_t> h_ccom;
};
// key-set FastAggregateVerify by random linear combination per message (host_keyset_rlc.hip, k_keyset_rlc.hip): the seed; per
// group its committee and row offset (committee form), sorted position, chunk-size byte, eligibility byte and weight; per sorted
// position its group; the weighted points A (27 x G limbs) and B (54 x G limbs) at their sorted positions with the (constant 1)
// flags k_g2_seg_sum reads; the chunks' starts and lengths, sums (27 / 54 x M limbs, with flags nobody reads), eligible counts,
// states and the encodings of their G1 sums; the list, points, flags, signatures, key encodings, messages, offsets and bits of a
// sub-call of the verify pipeline (the checked chunks, then the exact list); the levels of the sums.  Host side: the plan (its
// vectors are what the uploads read) and every copy an upload reads or a download fills.
struct BNH KsrWs {
  DevBuf seed, com, row_off, pos, order, multi, elig, wt, a, b, ones, cstart, clen, sa, sb, sb_ok, cnt, state, sa_bytes, list, c_pts, c_ok, c_sigs, pk, msgs,
         moff, bits;
  SegWs seg;
  KsrPlan plan;
  std::vector<uint8_t> h_elig, h_state, h_bits, h_msgs;
  std::vector<uint32_t> h_cstart, h_clen, h_list;
  std::vector<uint64_t> h_moff, h_rowoff;
  // groups decided by a passed chunk, chunks checked, groups sent to the exact path after their chunk failed, groups sent there directly, message classes, calls
  uint64_t stat[6] = {0, 0, 0, 0, 0, 0};
};
// aggregate verify over groups by random linear combination (host_aggregate_rlc.hip, k_aggregate_rlc.hip): the seed; per pair its
// group; the groups' pair offsets, segments, signature flags, eligibility bytes and weights; the weighted points
// (27 x W limbs: pairs, signatures, one identity per virtual key); per item its virtual key id; per virtual key the table it pairs
// with, its sum as an affine H point and the status of that; the segments' products and their is-one bytes; the groups' validity
// bytes; the levels of the segmented product.  Host side: the plan's vectors (what the uploads read), what a round downloads, and
// the bits of an exact sub-call.
struct BNH AgrWs {
  DevBuf seed, gidx, seg_of, sig_ok, elig, wt, w, vkid, mkid, h2, st, prod, isone, valid;
  GroupOff goff;
  SegWs seg;
  std::vector<uint32_t> h_gidx, h_bound, h_seg_of;
  std::vector<uint8_t> h_elig, h_pass, h_bits;
  std::vector<std::pair<size_t, size_t>> ranges;
  // calls, groups decided by round 1, by round 2, groups sent to the exact pipeline, ineligible groups, equations checked, calls that
  // did not take round 1, segments that failed
  uint64_t stat[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};
// pairing-product checks over groups by random linear combination (host_pairing_check_rlc.hip, k_pairing_check_rlc.hip): what a
// round needs is AgrWs's, an equation in place of a group and no signature items (gidx: per pair its equation; goff: the
// equations' pair offsets; sig_ok unused); on top of it the pairs' decoded P as affine limbs (18 x N) and the pairs' bytes.
// blsbn254_pairing_check_rlc_stats: AgrWs's counters index for index, with "equations of the call" for "groups"
struct BNH PcrWs : AgrWs { DevBuf pts, flag; };
// the distinct-message rule of the aggregate verify over groups (host_msg_distinct.hip, k_msg_distinct.hip): per pair the canonical
// (x, y) of its hash point (18 x N limbs), the slot table (M >= 2 N pair indices), the groups' repeat bytes and their bitmap; the
// group offsets of blsbn254_hash_distinct_batch (the verify calls pass their own).  Host side: the bitmap as downloaded.
// blsbn254_msg_distinct_stats, in its order: calls, pairs inserted, groups found repeated, slots of the last call
struct BNH MdWs {
  DevBuf key, slots, dup, bits;
  GroupOff goff;
  std::vector<uint8_t> h_bits;
  uint64_t stat[4] = {0, 0, 0, 0};
};
// sums of G1 points per key, level by level (host_rlc.hip key_sums; its users: the key round of rlc2_chunk_dev there,
// aggregate_verify_grouped of host_aggregate.hip and round 1 of host_aggregate_rlc.hip): per level (ping-pong) the keys' chunk
// counts, their prefix, the chunks' key ids and the chunk sums of one or two point arrays (27 x M limbs each); the chunks' starts
// and lengths and the items' chunk numbers of the level being summed; 0, 1, 2, ... as the item order of every level but the
// first.  Host side: the chunk count a level reads back.
struct BNH KeySumWs {
  DevBuf cnt[2], base[2], kid[2], start, len, tchunk, iota, out[2], out2[2];
  uint32_t h_m = 0;
};
// batch verification by random linear combination over repeated keys (host_rlc.hip rlc2_chunk_dev, k_rlc2.hip): the seed; the
// weighted points r_i sig_i and r_i H_i in key-sorted order (27 x n limbs each) and the signatures' flags; per tuple its chunk;
// per key its chunk count and the prefix of those; per chunk its key, start, length, sums (27 x m limbs each) and eligible count,
// and as a virtual tuple its signature encoding, H point, state and is-one byte; 0, 1, 2, ... over the chunks; the tuples'
// fallback marks with their block counts and prefix, the fallback list, the validity bytes.  The key round: per key its eligible
// count and, as a virtual tuple, its signature encoding, H point, state, is-one byte and verdict; per chunk the verdict its key's
// or its own check left, the mark "its key failed" with block counts and prefix, and the list of the marked chunks.  Host side,
// context-owned because asynchronous copies write them: the chunk count, the key round's verdict, the length of the chunk list,
// the fallback count; the seed of the call in flight (stage_seed uploads from it, for every RLC pipeline).  The settings, the
// back-off of the key round (rlc_plan.h) and the counters.
struct BNH Rlc2Ws {
  DevBuf seed, a, b, sigok, tchunk, ccnt, cbase, ckid, cstart, clen, sa, sb, celig, csig, ch, cstate, cisone, iota, need, bcnt, bbase, list, valid;
  DevBuf kelig, ksig, kh, kstate, kisone, kpass, cpass, cneed, cbcnt, cbbase, clist;
  uint32_t h_m = 0, h_mc = 0, h_m2 = 0;
  int h_all_pass = 0;
  uint8_t h_seed[32];
  size_t group = RLC_DEFAULT_GROUP;  // tuples per chunk (BLSBN254_RLC_GROUP / blsbn254_set_rlc_group)
  bool group_auto = true;            // no explicit setting: 16, raised (to at most 32) when that saves a whole round of waves (rlc_chunk_size)
  bool key_round = true;             // first check every key's whole run as ONE virtual tuple (BLSBN254_RLC_KEY_ROUND=0 disables)
  RlcBackoff backoff;                // ... backing off while batches keep failing it (the next 2, 4, 8, 16 calls skip it)
  // blsbn254_rlc_stats, in its order: tuples on the chunked path, chunks checked, tuples sent to the exact fallback, tuples on the
  // exact path (distinct keys), key rounds taken, key rounds passed
  uint64_t stat[6] = {0, 0, 0, 0, 0, 0};
};
// ... and its distinct-key variant (host_rlc.hip rlc_group_products / rlc_exact_failed, k_rlc.hip), groups of 16 tuples in the
// caller's order: the weighted points r_i sig_i (27 x n limbs, and the levels of their pairwise sums) and r_i H_i (18 x n limbs),
// the eligibility bytes; per group the Miller value of its signature sum, that sum's encoding, a -G2gen each, the is-one byte;
// for the exact sub-call over the groups that failed the tuples' indices and their gathered keys, signatures, H points, subgroup
// flags and bits.  Host side: the -G2gen tile the upload reads, what the two rounds download, the indices the upload reads.
// aggregate_verify_grouped (host_aggregate.hip) keeps its u + 1 H points in `b` and their key ids in `idx`: the two buffers
// serve whichever call runs, so the context's footprint is one of them, not two.
struct BNH RlcWs {
  DevBuf a2, a, b, elig, f2, bytes, neg, ok, idx, cpk, csig, ch, csub, cbm;
  std::vector<uint8_t> h_neg, h_ok, h_elig, h_bits;
  std::vector<uint32_t> h_idx;
};
// The final exponentiation (host.hip run_final_exp): the phase buffers (x, a, b, c, b2, d; 108 x n limbs each), the ten named
// powers of the t -> t^x addition chain (10 x 108 x n limbs), the validity bytes of the wave and quad hard parts (mode 0), the
// named values of the quad hard part (TRI_VALUES x 108 x n limbs)
struct BNH FeWs { DevBuf ph[6], slots, one, tri; };
// Key de-duplication of a chunk (host_verify.hip dedup_enqueue and what follows it): the hash table's slots, per tuple its
// representative and its key id, per distinct key its representative tuple, the keys' tuple counts, the run cursors (ends, after
// the scatter) and the key-sorted order, the key count.  Host side: the per-context random seed of the table's hash, and the id
// of -G2gen among a call's keys -- the one host copy an upload reads here (agg_keys_prepare), context-owned so nothing waits for it
struct BNH KeyDedupWs {
  DevBuf slots, rep, kid, keys, hist, cursor, perm, cnt;
  uint32_t seed = 0, last_key = 0;
};
// The prepared keys of a call (k_keyprep.hip, k_miller_prep.hip; prepare_keys, raw_tables_fork): the expanded pair tables, the raw
// line triples and the validity bytes of the keys prepared for this call; per tuple the is-one byte and the verdict byte of
// verify_prepared_dev.  No host copies.  blsbn254_path_stats, in its order: verify chunks that took the prepared-key path, the
// exact per-tuple path
struct BNH PrepWs {
  DevBuf table, raw, ok, isone, valid;
  uint64_t stat[2] = {0, 0};
};
// The store of prepared keys (key_cache.h, k_keycache.hip; host_verify.hip prepare_keys): the keys' encodings, pair tables and
// validity bytes, the slot table, the state words and running totals; per call the distinct keys' store indices, the miss list,
// and the store indices per tuple / per chunk of the RLC path, with the validity bytes in batch key order for that path
struct BNH KeyStore {
  DevBuf keys, table, valid, slots, state, slot_of, miss_rep, miss_slot, tslot, cslot, batch_ok;
  size_t max = 4096;                 // keys the store is made for (blsbn254_set_key_cache, BLSBN254_KEY_CACHE); 0: no store, every call prepares its keys
  size_t cap = 0;                    // keys the store has room for: max(max, the largest key capacity a call was enqueued with); 0: not set up
  uint32_t mask = 0;                 // slot-table entries - 1
};
// A blsbn254_verify_batch_dev call whose pipeline was enqueued on the previous call's key count and whose check has not been read
// back yet: the caller's device pointers, its tag (a copy: a re-run stages it again) and the event behind the check's copy
struct PendingVerify {
  const uint8_t *d_pks = nullptr, *d_msgs = nullptr, *d_sigs = nullptr; const uint64_t* d_off = nullptr;
  size_t n = 0; uint8_t* d_bitmap = nullptr; uint8_t dst[256]; size_t dst_len = 0; hipEvent_t ev = nullptr;
};
// The asynchronous verify queue (host_verify.hip verify_chunk_async / resolve_pending): up to four such calls, oldest first; their
// checks (u, ok) on the device and in the pinned host buffer the copies land in.  The events and the pinned buffer are created by
// the first asynchronous call and released by blsbn254_ctx_destroy.  The hints the capacity of the next call is chosen from, the
// switch, and blsbn254_async_stats in its order: chunks enqueued without a read-back, chunks re-run on the counting path
struct BNH VerifyQueue {
  PendingVerify pend[4];
  int head = 0, count = 0;
  uint32_t* host = nullptr;          // pinned, 4 slots x (u, ok)
  DevBuf dev;                        // the same on the device
  size_t u_hint = 0;                 // distinct keys of the last chunk that took the prepared path (0: none yet)
  size_t u_max_seen = 0;             // the largest key count a prepared chunk had on this context: the capacity never drops below it (a caller
                                     // alternating between a small and a large key set would otherwise re-run every large batch)
  bool async = true;                 // BLSBN254_ASYNC_VERIFY=0: every call reads the key count back before it enqueues the pipeline
  uint64_t stat[2] = {0, 0};
};
// Threshold combine of one group (host_aggregate.hip lagrange_enqueue / threshold_combine_one, k_threshold.hip): the decoded
// ids, the partial products of the Lagrange numerators and denominators, the coefficients as GLV halves, the window sums of the
// MSM and the buffer they are folded into
struct BNH ThWs { DevBuf x, num, den, glv, part, part2; };
// Segmented G2 sums (host_groupops.hip g2_group_sums; the key-set calls leave their sums here too): the loaded points and the
// groups' sums with their flags, the sums' encodings, the levels between points and sums
struct BNH G2SumWs { DevBuf items, items_ok, sum, sum_ok, pk; SegWs seg; };
// The check of dealt key shares (host_threshold_deal.hip, threshold_keycheck.h): the generator's multiples, built at the first
// check -- no workspace aliases them.  blsbn254_threshold_key_check_stats: launches of the check kernel, shares checked, builds of
// the table (0: not built yet)
struct BNH KeyCheckWs { DevBuf tab; uint64_t stat[3] = {0, 0, 0}; };
struct ProfEntry { uint64_t launches = 0; std::vector<std::pair<hipEvent_t, hipEvent_t>> pending; double ms = 0; };

// The context: two streams, the staging buffers every pipeline shares, one workspace per pipeline, the settings no single
// workspace owns, the profile.
struct blsbn254_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;     // the per-key preparation runs beside hash-to-G1
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool s2_pending = false;           // work was forked onto stream2 and the main stream has not waited for ev_join yet
  // Shared BY DESIGN, the property of whichever call runs: the call's inputs as uploaded (in_a keys / points, in_b signatures,
  // in_c messages, in_off their offsets; wire_a / wire_b: compressed keys / signatures, inflated into in_a / in_b by
  // host_compressed.hip), the tag, the H points (h_ws), the Miller values and their product levels (f_ws, f_ws2), the decoded keys
  // of the two-pairs-per-lane kernel (q_ws, 72 x lanes limbs), per-element flags, subgroup bytes and decode statuses (status_all:
  // of every chunk of a chunked call), the result bitmap, other outputs, scalars, and a few words of verdicts (misc)
  DevBuf in_a, in_b, in_c, in_off, dst, h_ws, f_ws, f_ws2, q_ws, flags, sub_ok, status, status_all, bitmap, out, scalars, misc;
  DevBuf wire_a, wire_b;
  uint8_t dst_host[256];  // the (pre-hashed if oversize) DST currently resident in `dst`, and its length; -1 = none
  int dst_host_len = -1;
  LaunchForms forms;                 // which device form runs at which size (launch_forms.h)
  uint32_t expander = BLSBN254_EXPAND_XMD_SHA256;   // the message expander every hashing launch runs under (blsbn254_set_expander; keccak.h EXPAND_*)
  uint32_t g1_map = BLSBN254_G1MAP_SVDW;            // the map behind every MESSAGE hashed to G1 (blsbn254_set_g1_map; lane_hash_tai.h G1MAP_*)
  size_t chunk = (size_t)1 << 22;    // tuples per launch of the chunked entry points (BLSBN254_CHUNK_LANES overrides: tests)
  bool auto_prepare = true;          // verify_batch / aggregate_verify: de-duplicate the public keys and prepare each distinct key once (BLSBN254_AUTO_PREPARE=0 disables)
  uint64_t agg_stat[2] = {0, 0};     // blsbn254_aggregate_path_stats: aggregate verifies served per distinct key, pair by pair
  size_t ksr_group = KSR_DEFAULT_GROUP;  // groups per chunk of the key-set RLC calls (blsbn254_set_keyset_rlc_group)
  size_t agr_segments = 0;           // blsbn254_set_aggregate_rlc_segments: 0 = the default rule, 1 = no second round, else S
  size_t pcr_segments = 0;           // blsbn254_set_pairing_check_rlc_segments: the same for blsbn254_pairing_check_batch_rlc
  int msm_window = 0;                // blsbn254_set_msm_window: 0 = chosen from n, 2..16 = forced (and the bucket path forced)
  FeWs fe;
  KeyDedupWs kd;                     // the verify path: key de-duplication,
  PrepWs prep;                       // ... the prepared keys of a call,
  KeyStore kc;                       // ... the store of prepared keys,
  VerifyQueue vq;                    // ... the asynchronous queue
  KeySumWs ks;                       // batch verification by random linear combination: the per-key sums,
  Rlc2Ws r2;                         // ... the rounds over repeated keys with their settings and counters,
  RlcWs rlc;                         // ... the distinct-key variant
  ThWs th;
  G2SumWs gs;
  MsmWs msm;
  PcWs pc;
  ThbWs thb;
  AgbWs agb;
  TdlWs tdl;
  KeyCheckWs kchk;
  TcWs tc;
  KsetWs kset;
  KaggWs kagg;
  KmWs kmrg;
  KwWs kw;
  KcWs kcom;
  KcaWs kcagg;
  KcmWs kcmrg;
  KsrWs ksr;
  AgrWs agr;
  PcrWs pcr;
  MdWs md;
  bool profiling = false;
  std::map<std::string, ProfEntry> prof;
  std::string last_error;
};

// THE body of a plain counter getter: the null checks, then the first n counters of the context's `stat` (kset.stat, ...) into out
#define COPY_STATS(c, stat, n, out) (!(c) || !(out) ? (int)BLSBN254_E_ARG : (std::copy_n((c)->stat, n, out), 0))

#define HIPCHK(ctx, x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { (ctx)->last_error = std::string(#x) + ": " + hipGetErrorString(e_); \
    return e_ == hipErrorOutOfMemory ? BLSBN254_E_NOMEM : BLSBN254_E_HIP; } } while (0)

// TRY(f(...)): a non-zero return code of f leaves the calling function, as ONE statement
#define TRY(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

static inline unsigned nblocks(size_t n) { return (unsigned)((n + 255) / 256); }
// Launch shapes, named where they are decided (a 2-D grid is written out as Shape{dim3(x, y), dim3(256)}):
struct Shape { dim3 grid, block; };
static inline Shape grid_lanes(size_t n) { return {dim3(nblocks(n)), dim3(256)}; }                   // one lane per element
static inline Shape grid_tri(size_t n) { return {dim3((unsigned)((n + 63) / 64)), dim3(256)}; }      // four lanes per element (tri.h): 256-lane workgroups of 64 elements
static inline Shape grid_wide(size_t n) { return {dim3((unsigned)n), dim3(128)}; }                   // two waves (wide.h: WIDE_LANES = 128) per element: the wave-per-tuple kernels
static const size_t TRI_VALUE_LIMBS = 20 * 108;      // tri.h TRI_VALUES x 108

// One timed launch of the profile (blsbn254_profile_read): an event pair around it on the stream it runs on.  name == nullptr: not profiled.
struct BNH ProfScope {
  blsbn254_ctx* c; hipStream_t s; const char* name; hipEvent_t e0 = nullptr, e1 = nullptr;
  ProfScope(blsbn254_ctx* c_, hipStream_t s_, const char* n) : c(c_), s(s_), name(c_->profiling ? n : nullptr) {
    if (name) { (void)hipEventCreate(&e0); (void)hipEventCreate(&e1); (void)hipEventRecord(e0, s); }
  }
  ~ProfScope() {
    if (name) { (void)hipEventRecord(e1, s); ProfEntry& p = c->prof[name]; ++p.launches; p.pending.emplace_back(e0, e1); }
  }
};
// THE way a kernel is launched on the host side: on stream s of the context, counted under `name`; 0 or the project's error code
template <typename... P, typename... A>
static inline int launch(blsbn254_ctx* c, hipStream_t s, const char* name, Shape g, void (*kernel)(P...), A... args) {
  { ProfScope ps(c, s, name); hipLaunchKernelGGL(kernel, g.grid, g.block, 0, s, args...); }
  HIPCHK(c, hipGetLastError());
  return 0;
}
// THE launches of the four hashing kernels, on the tag resident in c->dst (stage_dst: dl): the XMD-SHA-256 kernel under the
// default expander, its sibling of k_hash_keccak.hip under any other.  No host unit names those kernels but these four helpers,
// so every call that hashes follows blsbn254_set_expander.  Counted under one name whatever the expander.
// The two that hash a MESSAGE to G1 follow blsbn254_set_g1_map as well: under a try-and-increment map they launch the kernels of
// k_hash_tai.hip (the tag is passed and ignored).  encode_to_g1 (mode 2) keeps the RFC map, and so does every launch inside a
// RfcMapScope: the proofs of possession, whose tag is what separates them from messages.
static inline int launch_hash_to_g1(blsbn254_ctx* c, hipStream_t s, const uint8_t* msgs, const uint64_t* off, size_t n, uint32_t dl, int32_t* ws, size_t stride,
                                    uint8_t* out, int mode) {
  const uint8_t* dst = (const uint8_t*)c->dst.p;
  if (c->g1_map != BLSBN254_G1MAP_SVDW && mode != 2)
    return launch(c, s, "hash_to_g1", grid_lanes(n), k_hash_to_g1_tai, c->g1_map, c->expander, msgs, off, n, dst, dl, ws, stride, out, mode);
  if (c->expander == BLSBN254_EXPAND_XMD_SHA256) return launch(c, s, "hash_to_g1", grid_lanes(n), k_hash_to_g1, msgs, off, n, dst, dl, ws, stride, out, mode);
  return launch(c, s, "hash_to_g1", grid_lanes(n), k_hash_to_g1_x, c->expander, msgs, off, n, dst, dl, ws, stride, out, mode);
}
static inline int launch_hash_to_g2(blsbn254_ctx* c, hipStream_t s, const uint8_t* msgs, const uint64_t* off, size_t n, uint32_t dl, uint8_t* out, int ro) {
  const uint8_t* dst = (const uint8_t*)c->dst.p;
  if (c->expander == BLSBN254_EXPAND_XMD_SHA256) return launch(c, s, "hash_to_g2", grid_lanes(n), k_hash_to_g2, msgs, off, n, dst, dl, out, ro);
  return launch(c, s, "hash_to_g2", grid_lanes(n), k_hash_to_g2_x, c->expander, msgs, off, n, dst, dl, out, ro);
}
static inline int launch_sign(blsbn254_ctx* c, hipStream_t s, const uint8_t* sks, const uint8_t* msgs, const uint64_t* off, size_t n, uint32_t dl, uint8_t* sigs,
                              uint8_t* status) {
  const uint8_t* dst = (const uint8_t*)c->dst.p;
  if (c->g1_map != BLSBN254_G1MAP_SVDW) return launch(c, s, "sign", grid_lanes(n), k_sign_tai, c->g1_map, c->expander, sks, msgs, off, n, dst, dl, sigs, status);
  if (c->expander == BLSBN254_EXPAND_XMD_SHA256) return launch(c, s, "sign", grid_lanes(n), k_sign, sks, msgs, off, n, dst, dl, sigs, status);
  return launch(c, s, "sign", grid_lanes(n), k_sign_x, c->expander, sks, msgs, off, n, dst, dl, sigs, status);
}
static inline int launch_hash_to_scalar(blsbn254_ctx* c, hipStream_t s, const uint8_t* msgs, const uint64_t* off, size_t n, uint32_t dl, uint8_t* out) {
  const uint8_t* dst = (const uint8_t*)c->dst.p;
  if (c->expander == BLSBN254_EXPAND_XMD_SHA256) return launch(c, s, "hash_to_scalar", grid_lanes(n), k_hash_to_scalar, msgs, off, n, dst, dl, out);
  return launch(c, s, "hash_to_scalar", grid_lanes(n), k_hash_to_scalar_x, c->expander, msgs, off, n, dst, dl, out);
}
// The RFC 9380 map for the launches of one call, whatever the context's setting: held by the calls that hash a PUBLIC KEY under
// the proof-of-possession tag (pop_prove_batch, pop_verify_batch, the proof check of keyset_create_checked).  Taken AFTER ENTER
// (pending verify calls are settled under the caller's map) by calls that end synchronised, so nothing enqueued under it is
// re-run later.
struct BNH RfcMapScope {
  blsbn254_ctx* c; uint32_t was;
  explicit RfcMapScope(blsbn254_ctx* c_) : c(c_), was(c_->g1_map) { c->g1_map = BLSBN254_G1MAP_SVDW; }
  ~RfcMapScope() { c->g1_map = was; }
  RfcMapScope(const RfcMapScope&) = delete;
  RfcMapScope& operator=(const RfcMapScope&) = delete;
};
// reserve, then copy host -> device on the main stream (the source must outlive the copy: the caller's, or ctx-owned / static)
static inline int upload(blsbn254_ctx* c, DevBuf& b, const void* src, size_t bytes) {
  HIPCHK(c, b.reserve(bytes));
  HIPCHK(c, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
  return 0;
}
// copy device -> host behind everything enqueued on the main stream, and wait for it
static inline int download(blsbn254_ctx* c, void* dst, const void* src, size_t bytes) {
  HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
// body(lo, m) for every launch chunk [lo, lo + m) of n independent elements (ctx->chunk each, the last one shorter); stops at the
// first non-zero return code.  Chunk starts are multiples of 8: bitmap bytes do not straddle chunks.
template <typename F>
static inline int for_chunks(const blsbn254_ctx* c, size_t n, F body) {
  for (size_t lo = 0; lo < n; lo += c->chunk) TRY(body(lo, std::min(n - lo, c->chunk)));
  return 0;
}
// The levels of one launch of a segmented reduction, written once: level 0 reads `src`, every level but the last writes w's
// ping-pong buffers (flags only where the final destination has them), the last one writes `fin`.  level(src, start, len, m, out,
// last) launches one level's kernel over m runs; the descriptors are w's, staged by seg_stage.
struct SegSrc { const int32_t* v; size_t stride; const uint8_t* ok; };
struct SegDst { int32_t* v; size_t stride; uint8_t* ok; };
template <typename F>
static inline int seg_run_levels(const SegWs& w, const std::vector<SegLevel>& levels, SegSrc src, SegDst fin, F level) {
  int dst = 0;
  for (size_t lv = 0; lv < levels.size(); ++lv) {
    const SegLevel& P = levels[lv];
    const bool last = lv + 1 == levels.size();
    const SegDst out = last ? fin : SegDst{(int32_t*)w.seg[dst].p, P.count, fin.ok ? (uint8_t*)w.seg_ok[dst].p : nullptr};
    TRY(level(src, (const uint32_t*)w.start.p + P.first, (const uint32_t*)w.len.p + P.first, P.count, out, last));
    src = {out.v, out.stride, out.ok}; dst ^= 1;
  }
  return 0;
}
// G1Affine::identity on the wire: x = 0, y = 1
static inline void g1_identity_bytes(uint8_t o[64]) { std::memset(o, 0, 64); o[63] = 1; }
// ... and compressed (g1_compress of it): x = 0 with the parity of y = 1 as the flag
static inline void g1_identity_wire(uint8_t o[32]) { std::memset(o, 0, 32); o[0] = 0x80; }
// the identity in the encoding a call hands out: 32 bytes for the wire-format forms, 64 otherwise
static inline void g1_identity_out(uint8_t* o, bool wire) { if (wire) g1_identity_wire(o); else g1_identity_bytes(o); }

// Work forked onto stream2 must never outlive a failing call: a function that forks holds one of these, and an early
// error return (before the main stream has waited for ev_join) then waits for stream2 on the way out, so nothing is
// still writing prep.raw / prep.table when the caller sees the error code.
struct Stream2Guard {
  blsbn254_ctx* c;
  explicit Stream2Guard(blsbn254_ctx* c_) : c(c_) {}
  ~Stream2Guard() { if (c->s2_pending) { (void)hipStreamSynchronize(c->stream2); c->s2_pending = false; } }
};
static inline hipError_t fork_stream2(blsbn254_ctx* c) {
  hipError_t e = hipEventRecord(c->ev_fork, c->stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(c->stream2, c->ev_fork, 0);
  if (e == hipSuccess) c->s2_pending = true;
  return e;
}
static inline hipError_t join_stream2(blsbn254_ctx* c) {
  hipError_t e = hipStreamWaitEvent(c->stream, c->ev_join, 0);
  if (e == hipSuccess) c->s2_pending = false;
  return e;
}

extern "C" {
// every entry point: select the device, then settle what the asynchronous verify path left open (read back its checks, re-run a
// batch whose optimistic choice did not hold) -- results of earlier calls are final before this call touches the context
BNH int resolve_pending(blsbn254_ctx* c, bool blocking);   // host_verify.hip
BNH int blsbn254_internal_verify_batch_dev_sync(blsbn254_ctx* c, const uint8_t* d_pks, const uint8_t* d_msgs, const uint64_t* d_off,
                                                const uint8_t* d_sigs, size_t n, const uint8_t* dst, size_t dst_len, uint8_t* d_bitmap);   // host_verify.hip
#define ENTER(c) do { HIPCHK(c, hipSetDevice((c)->device)); if ((c)->vq.count) TRY(resolve_pending(c, true)); } while (0)
extern BNH const uint8_t NEG_G2_BYTES[128];     // -G2gen = (x, p - y) of the generator fp2.rs:305-333, as bytes (host.hip)

// The kernels address limb-major workspaces through a buffer descriptor with a 32-bit scalar byte offset
// (limb index x stride x 4, tower.h `Ws`): a launch may span at most MAX_LANES tuples (107 x 8 Mi x 4 B < 4 GiB).
// Independent-element entry points are processed in chunks of ctx->chunk (4 Mi); the product-type ones reject more.
static const size_t MAX_LANES = (size_t)1 << 23;
#define CHECK_LANES(c, n) do { if ((n) > MAX_LANES) { (c)->last_error = "more than 2^23 elements in one product-type call"; return BLSBN254_E_ARG; } } while (0)
// prepared-key path.  Limits: key ids and table offsets are 32-bit (88 x 54 x 4 B per key): at most PREP_MAX_KEYS keys.
static const size_t PREP_MAX_KEYS = (size_t)1 << 16;
static const size_t PREP_RAW_LIMBS = (size_t)BN_NEG_G2_LINES * 54;       // a key's 88 line triples
static const size_t PREP_KEY_LIMBS = (size_t)BN_NEG_G2_LINES * 162;      // a key's 88 expanded line pairs (key line x -G2gen line)
struct blsbn254_g2prepared { blsbn254_ctx* ctx; size_t u; DevBuf table, raw, ok; };   // pair tables (verify), raw line triples (multi_miller_loop), validity
// a registered key set (host_keyset.hip): the keys as affine limb-major rows (36 x n limbs), the bad / skip words (keyset.h), the
// total of the non-skipped keys (54 limbs), KeyValidate per key (bytes), the encodings as they were uploaded (128 B per key: the
// per-signature fallback of host_keyset_agg.hip gathers its keys from them), the KeyValidate bits packed into a word per 32 keys
// (bits past the last key 0: the selection of host_keyset_merge.hip tests a row's words against them).  A set registered with
// proofs of possession (checked): the bits of the proofs' verification, which the registration folds into bad / skip / valid.
// The stake table (host_keyset_weight.hip; n_cols == 0: none): key-major, weff[i * n_cols + q] = column q of key i (the kernel
// masks every row with vwords, so a key without the KeyValidate bit weighs 0), and the columns' totals of the effective weights
// The committee table (host_keyset_committee.hip; no committees: none): the members' key indices, the committees as the kernels
// read them (KcCom), per committee word the bad / skip / valid bits of its members (keyset_committee.h), per committee the total
// of its non-skipped members (54 limbs, limb-major with stride n_com); the host mirror for argument checks and planning.
struct BNH KcDev {
  DevBuf members, coms, cbad, cskip, cvalid, totals;
  KcTable tab;
  void swap(KcDev& o) {
    DevBuf* a[6] = {&members, &coms, &cbad, &cskip, &cvalid, &totals};
    DevBuf* b[6] = {&o.members, &o.coms, &o.cbad, &o.cskip, &o.cvalid, &o.totals};
    for (int i = 0; i < 6; ++i) { std::swap(a[i]->p, b[i]->p); std::swap(a[i]->cap, b[i]->cap); }
    std::swap(tab, o.tab);
  }
};
struct blsbn254_keyset {
  blsbn254_ctx* ctx; size_t n; DevBuf aff, bad, skip, total, valid, enc, vwords;
  bool checked = false; DevBuf pop;
  size_t n_cols = 0; DevBuf weff; uint64_t wtotal[BLSBN254_KS_MAX_COLS] = {};
  KcDev cm;
};

// ---- internal helpers shared between the units (defined in the unit named on the right)
BNH int stage_dst(blsbn254_ctx* c, const uint8_t* dst, size_t dst_len, uint32_t* out_len);   // host.hip
BNH int check_offsets(const uint64_t* off, size_t n);   // host.hip
// "The minimum index that fails, or none": k_status_reduce / k_kd_hist fold failing indices with atomicMin into an int that starts
// at NO_INDEX.  min_index_arm enqueues that start value for `words` (<= 2) ints at d, from a static source; min_index_read copies
// one back, waits, and reports -1 for none.
static const int NO_INDEX = 0x7fffffff;
BNH int min_index_arm(blsbn254_ctx* c, int* d, size_t words);   // host.hip
BNH int min_index_read(blsbn254_ctx* c, const int* d, int* out);   // host.hip
BNH int first_bad(blsbn254_ctx* c, const uint8_t* d_status, size_t n, uint8_t mask, uint8_t val, int* out);   // host.hip
BNH int read_status(blsbn254_ctx* c, const uint8_t* d_status, int idx, uint8_t* st);   // host.hip
BNH int run_final_exp(blsbn254_ctx* c, int32_t* f, size_t n, size_t stride, int mode, const uint8_t* flags, const uint8_t* sub_ok,
                         uint8_t* d_bitmap, uint8_t* d_gt, int* d_is_one);   // host.hip
BNH int miller_to_ws(blsbn254_ctx* c, const uint8_t* d_g1, const uint8_t* d_g2, size_t n);   // host.hip
BNH int decode_status_rc(blsbn254_ctx* c, const uint8_t* d_status, size_t n);   // host.hip
BNH int stage_msgs(blsbn254_ctx* c, const uint8_t* msgs, const uint64_t* off, size_t n);   // host.hip
BNH int launch_g2_prepare(blsbn254_ctx* c, hipStream_t s, const uint8_t* pks, const uint32_t* keys, size_t u, int32_t* raw, uint8_t* ok, const uint32_t* d_u);   // host_verify.hip
// A batch's prepared keys as their consumers see them: the entry of batch key j in table / ok is slot_of ? slot_of[j] : j.
// prepare_keys fills one for the keys left by dedup_keys / dedup_enqueue, from the context's store or prepared for this call, on
// stream2 with ev_join behind it (cap: the key count the call is enqueued with; d_u, optional: the count on the device when cap is
// only a capacity); the explicit G2Prepared API builds one with slot_of = nullptr.  Consumers do not ask which: key_miller_ids /
// miller_ids give the ids the Miller loops take (of the keys themselves -- iota = 0, 1, ... serves without a store -- and of
// elements given by batch key id, mapped into buf with one), keys_valid the validity bytes in batch key order (after join_stream2).
struct KeyTables { const int32_t* table; const uint8_t* ok; const uint32_t* slot_of; };
static inline const uint32_t* key_miller_ids(const KeyTables& kt, const uint32_t* iota) { return kt.slot_of ? kt.slot_of : iota; }
BNH int prepare_keys(blsbn254_ctx* c, const uint8_t* d_pks, size_t cap, const uint32_t* d_u, KeyTables* kt);   // host_verify.hip
BNH int miller_ids(blsbn254_ctx* c, const KeyTables& kt, const uint32_t* ids, size_t n, DevBuf& buf, const uint32_t** out);   // host_verify.hip
BNH int keys_valid(blsbn254_ctx* c, const KeyTables& kt, size_t u, const uint8_t** out);   // host_verify.hip
// behind dedup_keys / dedup_enqueue: key ids (kd.kid; hist: their counts, kd.hist), then the key-sorted order of d_kid (kd.perm, kd.cursor)
BNH int dedup_key_ids(blsbn254_ctx* c, size_t n, size_t u, bool hist);   // host_verify.hip
BNH int key_sorted_order(blsbn254_ctx* c, const uint32_t* d_kid, size_t n, size_t u);   // host_verify.hip
BNH int verify_prepared_dev(blsbn254_ctx* c, const KeyTables& kt, size_t u, const uint32_t* d_kid, bool deduped, const uint8_t* d_msgs, const uint64_t* d_off,
                            const uint8_t* d_sigs, size_t n, uint32_t dl, uint8_t* d_bitmap);   // host_verify.hip
BNH int check_key_indices(blsbn254_ctx* c, const uint32_t* d_kid, size_t n, size_t u, uint32_t* hist, const char* what, bool armed);   // host_verify.hip
BNH int launch_miller_prepared(blsbn254_ctx* c, const uint32_t* perm, const uint32_t* kid, const uint8_t* sigs, const int32_t* h_ws, size_t h_stride, const KeyTables& kt, size_t n);   // host_verify.hip
// Its twin over the RAW line tables (prep.raw / a G2Prepared's raw: the aggregate family): pair i = (H point i of the workspace h
// at stride h_stride, table kid[i] of kt), st: the optional status bytes of the H points (bit 1: the identity, contributes 1).
// Reserves and fills c->f_ws / c->flags; *left Fp12 values at stride *left remain: n, or (n + 1) / 2 from two pairs per lane.
// The form is launch_forms.h's (table_miller_form / raw_two_per_lane) over the forms the site admits (MR_*); n > ctx->chunk: the
// per-pair forms run chunk by chunk at stride n, each chunk in the form that fits it.
struct RawTables { const int32_t* raw; const uint8_t* ok; };
BNH int launch_miller_raw(blsbn254_ctx* c, const int32_t* h, size_t h_stride, const uint32_t* kid, RawTables kt, size_t n, const uint8_t* st, unsigned forms,
                          size_t* left);   // host_aggregate.hip
// The key tables of an aggregate call, in two steps because the callers decide between them whether to go on at all.
// agg_keys_stage: the caller's n keys into c->in_a with -G2gen as entry n, de-duplicated (dedup_keys: *u distinct among the n;
// synchronises).  agg_keys_prepare: -G2gen appended as key u, the raw tables of the u + 1 keys enqueued on the second stream beside
// whatever the caller enqueues next, ev_join recorded (raw_tables_fork: the same for the `keys` keys kd.keys names as it stands).
BNH int agg_keys_stage(blsbn254_ctx* c, const uint8_t* pks, size_t n, size_t* u);   // host_aggregate.hip
BNH int agg_keys_prepare(blsbn254_ctx* c, size_t n, size_t u);   // host_aggregate.hip
BNH int raw_tables_fork(blsbn254_ctx* c, size_t keys);   // host_aggregate.hip
// One round of a verify by random linear combination over the weighted points of w.w (stride W; host_aggregate_rlc.hip): the N
// pairs' items (and, sig_slots: the G signatures') get the virtual key id segment * u + key id, are summed per virtual key and
// paired with their keys' raw tables; the is-one byte of every segment's product into w.h_pass (synchronised).  d_seg_of: the
// groups' segments on the device, nullptr for S == 1.  sig_slots: blsbn254_aggregate_verify_batch_rlc's round (V = S (u + 1): a
// signature slot per segment on table u); without them (G is not read) blsbn254_pairing_check_batch_rlc's, V = S u.
BNH int agr_round(blsbn254_ctx* c, AgrWs& w, size_t N, size_t G, size_t u, size_t S, size_t W, const uint32_t* d_seg_of, bool sig_slots);
// valid = eligible (w.elig) and the segment's equation held (w.isone), packed into c->bitmap and downloaded
BNH int agr_bits(blsbn254_ctx* c, AgrWs& w, size_t G, const uint32_t* d_seg_of, uint8_t* bm);
// what blsbn254_aggregate_verify_batch and ..._batch_rlc check alike (`call` names the one in the error text); CK_NOTHING: no
// groups, the caller returns 0
// ... and the part of it that a call over ragged groups of MESSAGES alone shares (blsbn254_hash_distinct_batch): the context,
// n_groups == 0, the group and message offsets, the tag, the limits.  missing: an argument of the form's own that every call
// needs (its outputs, the signatures) is NULL; pair_missing: one that a call with pairs needs (the keys) is.  Neither is read.
BNH int agg_msg_args(blsbn254_ctx* c, const uint8_t* msgs, const uint64_t* off, const uint64_t* grp_off, size_t n_groups, const uint8_t* dst, size_t dst_len,
                     bool missing, bool pair_missing, const char* call);   // host_aggregate_batch.hip
BNH int agg_batch_args(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, const uint64_t* grp_off, const uint8_t* agg_sigs,
                       size_t n_groups, const uint8_t* dst, size_t dst_len, const uint8_t* valid_bitmap, const char* call);   // host_aggregate_batch.hip
// The distinct-message rule as ONE stage (host_msg_distinct.hip; enqueued): the N points at pts (limb-major, stride `stride`,
// form MD_AFFINE: x, y / MD_HOMOGENEOUS: x, y, z) of the G groups whose rebased pair offsets lie at d_goff on the device; leaves
// c->md.dup[g] = 1 for every group with two pairs of the same point.  The table and dup[] are cleared on the stream first.
BNH int msg_distinct_stage(blsbn254_ctx* c, const int32_t* pts, size_t stride, size_t N, int form, const uint32_t* d_goff, size_t G);
// ... and its result on the host: c->md.dup packed LSB-first into c->md.h_bits (ceil(G / 8) bytes; synchronises), copied to
// dup_bitmap unless that is NULL; counts the call
BNH int msg_distinct_bits(blsbn254_ctx* c, size_t N, size_t G, uint8_t* dup_bitmap);
// the bodies of blsbn254_aggregate_verify_batch and ..._batch_rlc, argument checks included (`call` names the entry point in the
// error text): want_dup runs the stage on the hash points of the pipeline and leaves the groups' repeat bits in c->md.h_bits
// (valid_bitmap is NOT masked here: the _distinct entry points do that); without it they are the calls they were
BNH int aggregate_verify_batch_impl(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, const uint64_t* grp_off,
                                    const uint8_t* agg_sigs, size_t n_groups, const uint8_t* dst, size_t dst_len, uint8_t* valid_bitmap, bool want_dup,
                                    const char* call);   // host_aggregate_batch.hip
BNH int aggregate_verify_batch_rlc_impl(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, const uint64_t* grp_off,
                                        const uint8_t* agg_sigs, size_t n_groups, const uint8_t* dst, size_t dst_len, const uint8_t* seed,
                                        uint8_t* valid_bitmap, bool want_dup, const char* call);   // host_aggregate_rlc.hip
BNH int dedup_keys(blsbn254_ctx* c, const uint8_t* d_pks, size_t n, size_t* u_out);   // host_verify.hip
BNH int verify_exact_dev(blsbn254_ctx* c, const uint8_t* d_pks, const uint8_t* d_msgs, const uint64_t* d_off,
                            const uint8_t* d_sigs, size_t n, uint32_t dl, uint8_t* d_bitmap);   // host_verify.hip
BNH int verify_chunk_dev(blsbn254_ctx* c, const uint8_t* d_pks, const uint8_t* d_msgs, const uint64_t* d_off,
                            const uint8_t* d_sigs, size_t n, uint32_t dl, uint8_t* d_bitmap);   // host_verify.hip
// segmented sums of n G2 encodings staged at d_pks over the groups goff (host offsets) into c->gs.sum / c->gs.sum_ok
BNH int g2_group_sums(blsbn254_ctx* c, const uint8_t* d_pks, size_t n, const uint64_t* goff, size_t n_groups);   // host_groupops.hip
// the sums of n_groups rows ALREADY ON THE DEVICE (ceil(k->n / 8) bytes each) over the key set k into c->gs.sum / c->gs.sum_ok,
// the flip bytes into c->kset.h_flip (enqueued); *launches: launches of the word kernel
BNH int ks_enqueue_sums_dev(blsbn254_ctx* c, const blsbn254_keyset* k, const uint8_t* d_rows, size_t n_groups, size_t* launches);   // host_keyset.hip
// the argument checks the calls over rows share (n_groups > 0): the limit, and no row may set a bit that names no key
BNH int ks_args(blsbn254_ctx* c, const blsbn254_keyset* k, const uint8_t* sel, size_t n_groups);   // host_keyset.hip
// blsbn254_keyset_fast_aggregate_verify_batch behind its argument checks and ENTER; sel == nullptr: the rows are in c->kset.sel already
// compressed: the signatures are 32-byte encodings (stage_g1)
BNH int ks_verify_rows(blsbn254_ctx* c, const blsbn254_keyset* k, const uint8_t* sel, const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs,
                       size_t n_groups, const uint8_t* dst, size_t dst_len, uint8_t* valid_bitmap, bool compressed = false);   // host_keyset.hip
// A call's n public keys into c->in_a / its n signatures into c->in_b, where every pipeline reads them: uploaded as they are, or
// (compressed: 64 / 32 bytes each) uploaded to c->wire_a / c->wire_b and inflated from there by k_g2_inflate / k_g1_inflate,
// an element that does not inflate as the marker no decoder accepts (inflate.h).  Enqueued.
BNH int stage_g2(blsbn254_ctx* c, const uint8_t* pks, size_t n, bool compressed);    // host_compressed.hip
BNH int stage_g1(blsbn254_ctx* c, const uint8_t* sigs, size_t n, bool compressed);   // host_compressed.hip
// n 32-byte signatures ALREADY ON THE DEVICE at d_in inflated into the 64 n bytes at d_out (k_g1_inflate, launch chunk by launch
// chunk; enqueued): for the callers that stage signatures in buffers of their own
BNH int g1_inflate_dev(blsbn254_ctx* c, const uint8_t* d_in, size_t n, uint8_t* d_out);   // host_compressed.hip
// the entry points that exist in both forms, behind their argument checks and ENTER
BNH int verify_batch_host(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs, size_t n, const uint8_t* dst,
                          size_t dst_len, uint8_t* bm, bool compressed);   // host_verify.hip
BNH int verify_batch_rlc_host(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs, size_t n, const uint8_t* dst,
                              size_t dst_len, const uint8_t* seed, uint8_t* bm, bool compressed);   // host_rlc.hip
// the registration of a key set, arguments checked in here; proofs == nullptr: without proofs of possession
BNH int ks_create(blsbn254_ctx* c, const uint8_t* pks, const uint8_t* proofs, size_t n_keys, const uint8_t* pop_dst, size_t pop_dst_len,
                  blsbn254_keyset** out, bool compressed);   // host_keyset.hip
// the tail of ks_verify_rows: the sums in c->gs.sum / c->gs.sum_ok (enqueued) encoded and paired with the staged messages and
// signatures (stage_msgs, c->in_b), the bits downloaded
BNH int ks_verify_sums(blsbn254_ctx* c, size_t n_groups, uint32_t dl, uint8_t* valid_bitmap);   // host_keyset.hip
// the committee form's sums: the arguments checked (n_groups > 0), then the rows staged in c->kcom.sel, the sums into c->gs.sum /
// c->gs.sum_ok in the caller's order (enqueued); kc_tally counts the call once it has succeeded and synchronised
BNH int kc_args(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* com, const uint8_t* sel, const uint64_t* sel_off, size_t n_groups);   // host_keyset_committee.hip
BNH int kc_enqueue_call(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* com, const uint8_t* sel, const uint64_t* sel_off, size_t n_groups);   // host_keyset_committee.hip
BNH void kc_tally(blsbn254_ctx* c, size_t n_groups);   // host_keyset_committee.hip
// kc_enqueue_call behind its upload: the rows are ALREADY ON THE DEVICE at d_rows, row g at d_rows + (sel_off[g] - sel_off[0])
BNH int kc_enqueue_call_dev(blsbn254_ctx* c, const blsbn254_keyset* k, const uint32_t* com, const uint8_t* d_rows, const uint64_t* sel_off, size_t n_groups);   // host_keyset_committee.hip
// the full-width form's: the rows staged in c->kset.sel, the sums enqueued; ks_tally counts the call likewise
BNH int ks_enqueue_sums(blsbn254_ctx* c, const blsbn254_keyset* k, const uint8_t* sel, size_t n_groups, size_t* launches);   // host_keyset.hip
BNH void ks_tally(blsbn254_ctx* c, size_t n_groups, size_t launches);   // host_keyset.hip
BNH int key_sums(blsbn254_ctx* c, const int32_t* pts, const int32_t* pts2, size_t pts_stride, const uint32_t* mark_perm, const uint32_t* pt_perm,
                    const uint32_t* kid, const uint32_t* hist, const uint32_t* run_end, size_t items, size_t u, const int32_t** out, const int32_t** out2);   // host_rlc.hip
// THE seed stage of the RLC pipelines: the caller's seed, or 32 bytes drawn from the OS now -- after the batch is fixed -- into
// c->r2.h_seed (context-owned: it outlives the copy) and from there into d.  Enqueued.
BNH int stage_seed(blsbn254_ctx* c, DevBuf& d, const uint8_t* seed);   // host_rlc.hip
BNH int prepared_round(blsbn254_ctx* c, const uint32_t* perm, const uint32_t* kid, const KeyTables& kt, const uint8_t* sigs, const int32_t* h_ws, size_t h_stride, size_t cnt, uint8_t* d_isone);   // host_rlc.hip
// The segmented reductions' device side.  seg_stage: w's ping-pong buffers for levels of at most items_max items of `limbs` limbs
// (with `flags`, a byte per item too) and the upload of the descriptors planned into w.h_start / w.h_len.
BNH int seg_stage(blsbn254_ctx* c, SegWs& w, size_t items_max, size_t limbs, bool flags);   // host_seg.hip
// the caller's offsets off[0 .. n_groups], rebased to 0, into o.h and o.d (enqueued); more than MAX_LANES elements: an internal error
BNH int stage_group_offsets(blsbn254_ctx* c, GroupOff& o, const uint64_t* off, size_t n_groups);   // host_seg.hip
// pairing products, shared with the aggregate verify over groups (host_pairing_check.hip): the products' buffers and the staging
// of c->pc.seg for a planned call (the callers run the levels, seg_run_levels with k_fp12_seg_prod, into c->pc.prod / c->pc.ok);
// the products' final exponentiation into the bitmap, by chunks of equations
static const size_t FP12_SEG_GROUP = 8;     // Miller values per lane of the segmented product
BNH int pc_reserve_products(blsbn254_ctx* c, size_t n_eq, size_t items_max);
BNH int pc_finish_bitmap(blsbn254_ctx* c, size_t n_eq, uint8_t* valid_bitmap);
// the argument checks of the calls over ragged groups of pairs (n_eq > 0, c not NULL; `out`: the call's output)
BNH int pc_args(blsbn254_ctx* c, const uint8_t* g1, const uint8_t* g2, const uint64_t* off, size_t n_eq, const void* out);
BNH int fp12_tree(blsbn254_ctx* c, int32_t* a, size_t cnt, size_t sa, int32_t** res, size_t* rs);   // host_aggregate.hip
BNH int g1_sum_to_bytes(blsbn254_ctx* c, size_t n, uint8_t out[64]);   // host_aggregate.hip
BNH int threshold_combine_one(blsbn254_ctx* c, const uint8_t* ids, const uint8_t* partial_sigs, size_t t, uint8_t out_sig[64]);   // host_aggregate.hip
BNH int lagrange_one(blsbn254_ctx* c, const uint8_t* ids, size_t t, uint8_t* out);   // host_aggregate.hip
// threshold combine over groups on ids / partial signatures ALREADY ON THE DEVICE (d_sigs == null: the coefficients alone); off:
// host offsets as the entry points take them.  Enqueues only: statuses into c->thb.st, encodings into c->thb.out.
BNH int th_enqueue_dev(blsbn254_ctx* c, const uint8_t* d_ids, const uint8_t* d_sigs, const uint64_t* off, size_t n_groups);   // host_threshold_batch.hip
BNH size_t th_batch_tbig();   // host_threshold_batch.hip: the largest group the lane-per-share kernels serve
// the argument checks the dealing-side entry points share, and the device part of blsbn254_threshold_verify_shares_batch: the
// shares' bits into c->bitmap, the groups' statuses into c->tdl.st (enqueued; the caller downloads and synchronises)
BNH int td_args(blsbn254_ctx* c, const void* coefs, const uint64_t* coef_off, const uint8_t* ids, const uint64_t* id_off, size_t n_groups, const void* out,
                const void* status);   // host_threshold_deal.hip
// the checks of the arguments that come with one message per group (after td_args; same codes and text in both callers)
BNH int td_msg_args(blsbn254_ctx* c, const uint8_t* partial_sigs, const uint64_t* id_off, const uint8_t* msgs, const uint64_t* msg_off, size_t n_groups,
                    const uint8_t* dst, size_t dst_len);   // host_threshold_deal.hip
// the call's commitments uploaded, loaded and tested into c->tdl (coef, c_ws, c_ok, c_sub); enqueued
BNH int td_stage_commitments(blsbn254_ctx* c, const uint8_t* commitments, const uint64_t* coef_off, size_t n_groups);   // host_threshold_deal.hip
BNH int td_verify_shares_enqueue(blsbn254_ctx* c, const uint8_t* commitments, const uint64_t* coef_off, const uint8_t* ids, const uint8_t* partial_sigs,
                                 const uint64_t* id_off, const uint8_t* msgs, const uint64_t* msg_off, size_t n_groups, const uint8_t* dst, size_t dst_len);   // host_threshold_deal.hip
// The checked calls over a registered key set (host_keyset_agg / _merge / _committee_agg / _committee_merge.hip): the steps all
// four share, each written once in host_keyset_checked.hip.  CkArgs: the arguments they share, sigs indexed by ent_off as given
// (wire: 32 bytes per signature in and per sum out); CkOut: the caller's outputs (used: merge forms, else NULL).
static const size_t CK_SUM_GROUP = 16;      // signatures per lane and level of the group sums
static inline bool bit_at(const uint8_t* bm, size_t i) { return (bm[i >> 3] >> (i & 7)) & 1; }
static inline void set_bit(uint8_t* bm, size_t i) { bm[i >> 3] |= (uint8_t)(1u << (i & 7)); }
struct CkArgs {
  const uint8_t* sigs; const uint64_t* ent_off; const uint8_t* msgs; const uint64_t* msg_off;
  size_t n_groups;
  const uint8_t* dst; size_t dst_len;
  bool wire;
};
struct CkOut { uint8_t *sigs, *rows, *used, *status; };
// the sub-call a form's repack leaves: its entries, the byte offsets of its groups' rows and (merge forms, else NULL) per entry
// its index in the caller's arrays with the groups' entry offsets
struct CkSub { size_t n; const uint64_t* row_off; const uint64_t *pos, *off; };
// The argument checks: context and handle, n_groups == 0 (CK_NOTHING: the caller returns 0), NULL pointers (missing: one of the
// form's own or of its outputs is; ent_missing: one that a call with entries needs is), committees: the handle needs a table,
// the chunk limit, the offsets ("<noun> offsets decrease")
static const int CK_NOTHING = 1;
BNH int ck_args(blsbn254_ctx* c, const blsbn254_keyset* k, const CkArgs& A, bool missing, bool ent_missing, bool committees, const char* noun);
// the call's N signatures into w.sigs, through w.wire and g1_inflate_dev when compressed; inflate = false: compressed entries stay
// in w.wire, where the caller's scan reads them, and no 64 N buffer is reserved
BNH int ck_stage_sigs(blsbn254_ctx* c, CkWs& w, const CkArgs& A, size_t N, bool inflate);
// c->gs.pk / gs.sum / gs.sum_ok for n key sums: a call that uses them twice reserves for the larger use BEFORE the first kernel
// that touches them is enqueued (a later reserve that grows them would free what that kernel still reads)
BNH int ck_reserve_key_sums(blsbn254_ctx* c, size_t n);
// the group's message once per entry of w.goff into w.s_emsgs / w.s_emoff (ctx-owned: they outlive the upload)
BNH void ck_expand_msgs(CkWs& w, const CkArgs& A);
// the tail of an attempt, behind the kernels that left the entries' points in w.pts and the rows in w.orows: the signature sums by
// levels, their encodings into w.out (wire: w.wout too), the key sums by key_sums() into c->gs.sum / c->gs.sum_ok, then ONE
// verification per group of (key sum, message, signature sum), its bits into w.gbits.  Enqueued.
BNH int ck_tail(blsbn254_ctx* c, CkWs& w, const CkArgs& A, uint32_t dl, const std::function<int()>& key_sums);
// The two attempts of a call: attempt(false) over the caller's groups, the download, the groups marked; for those that had a
// candidate and failed the sub-call's messages (w.s_msgs / w.s_moff, final before the repack runs, so it may point its call at
// them), the form's repack(fail), their rows zeroed, attempt(true) and what passes copied back.  row_off: the
// byte offsets of the groups' rows in O.rows (rebased here; ck_even_rows for rows of one width); stat: the form's four counts.
BNH int ck_two_attempts(blsbn254_ctx* c, CkWs& w, const CkArgs& A, const uint64_t* row_off, const CkOut& O, uint64_t stat[4],
                        const std::function<int(bool)>& attempt, const std::function<CkSub(const std::vector<size_t>&)>& repack);
BNH const uint64_t* ck_even_rows(CkWs& w, size_t n_groups, size_t row_bytes);
// the aggregation pair's per-signature verification: the keys d_idx names gathered from the handle's encodings into pks, the
// group's message once per entry, the bits into w.vbits (synchronises)
BNH int ck_verify_entries(blsbn254_ctx* c, const blsbn254_keyset* k, CkWs& w, DevBuf& pks, const uint32_t* d_idx, const CkArgs& A, size_t N);
// the merge pair's selection: the signature test (k_km_sig), select(lo, m) for every launch of a wave per group, the points of
// what was not selected cleared and the used / candidate bitmaps (k_km_points)
BNH int ck_select(blsbn254_ctx* c, KmStage& w, size_t n_groups, size_t N, const std::function<int(size_t, size_t)>& select);
// ... and its per-contribution verification: key_sums(lo, m) for every launch chunk, the group's message once per contribution,
// the bits into w.vbits; settle: wait for each launch before the next is planned
BNH int ck_verify_contributions(blsbn254_ctx* c, KmStage& w, const CkArgs& A, size_t N, uint32_t dl, bool settle,
                                const std::function<int(size_t, size_t)>& key_sums);

}  // extern "C"
