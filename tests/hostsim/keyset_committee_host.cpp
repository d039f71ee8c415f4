// keyset_committee_host.cpp -- the lane functions of csrc/keyset_committee.h (committees over a registered key set) and the plain
// C++ of csrc/keyset_committee_plan.h compiled for the host with -DBN_CHECK, for tests/test_keyset_committee_host.py.  A
// STAND-ALONE program: it reads commands from the file named on its command line and prints one line of results per command, so
// a host sanitizer build of it (-fsanitize=address,undefined) runs as it is.  It keeps ONE committee table, as a handle does: `set`
// builds a new one beside it and replaces it only when every check passes.  The kernels of k_keyset_committee.hip are run lane by
// lane as they index their arguments; the segmented reduction is run from the descriptors of plan_seg_levels as k_g2_seg_sum
// reads them.  TEST TOOL ONLY.
//   set     n_keys n_com off(n_com+1) members(M)      -> "ok" or "refused", the committees of the table now kept, the error text
//   plan    chunk n_groups com(n_groups)              -> n_launches n_items order spbase srow, per launch lo hi item0 n_items
//                                                        partials levels, per item cword mbase first count
//   words   n_keys bad(hex, a byte per key) skip valid -> the table's cbad, cskip and cvalid words
//   count   size noflip row(hex) cbad(words)          -> flip ok
//   rows    n_groups com(n_groups) rows(hex)          -> -1 or the first group kc_check_rows refuses
//   sum     n_keys chunk n_groups com(n_groups) pks(hex) rows(hex)
//                                                      -> per group flip ok and the 128 bytes of its sum (hex), then the launches
// Blobs are hex strings, "-" for an empty one; numbers are decimal.
#include "../../bls-bn254_amd/csrc/keyset_committee.h"
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>

using namespace bn;

static std::vector<uint8_t> blob(std::istream& in) {
  std::string s;
  in >> s;
  std::vector<uint8_t> v;
  if (s == "-") return v;
  for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  return v;
}
template <typename T>
static std::vector<T> nums(std::istream& in, size_t n) {
  std::vector<T> v(n);
  for (size_t i = 0; i < n; ++i) { uint64_t x; in >> x; v[i] = (T)x; }
  return v;
}
static std::vector<uint32_t> pack_words(const std::vector<uint8_t>& bytes, uint32_t n_keys) {
  std::vector<uint32_t> v(ks_words(n_keys), 0);
  for (uint32_t i = 0; i < n_keys; ++i)
    if (bytes[i]) v[i >> 5] |= 1u << (i & 31);
  return v;
}
// the row offsets of a call whose rows follow one another
static std::vector<uint64_t> row_offsets(const KcTable& t, const std::vector<uint32_t>& com) {
  std::vector<uint64_t> off(1, 0);
  for (uint32_t c : com) off.push_back(off.back() + kc_row_bytes(t.com[c].size));
  return off;
}

static KcTable cur;
static std::vector<uint32_t> cur_members;

// k_kc_words over the whole table
static void run_words(const uint32_t* bad, const uint32_t* skip, const uint32_t* valid, std::vector<uint32_t>& cbad, std::vector<uint32_t>& cskip,
                      std::vector<uint32_t>& cvalid) {
  cbad.assign(cur.words, 0); cskip.assign(cur.words, 0); cvalid.assign(cur.words, 0);
  for (size_t cw = 0; cw < cur.words; ++cw) {
    const KcCom& k = cur.com[cur.wcom[cw]];
    const uint32_t w = (uint32_t)cw - k.wbase;
    const KcBits b = kc_word_bits(cur_members.data() + k.off + 32 * w, kc_left(k.size, w), bad, skip, valid);
    cbad[cw] = b.bad; cskip[cw] = b.skip; cvalid[cw] = b.valid;
  }
}
// kc_enqueue_sums of host_keyset_committee.hip: the reduced sum of every sorted group, flip / ok by sorted position
static void run_sums(const KcPlan& P, const std::vector<uint32_t>& start, const std::vector<uint32_t>& len, const std::vector<int32_t>& aff, uint32_t n_keys,
                     const std::vector<uint32_t>& cbad, const std::vector<uint32_t>& cskip, const uint8_t* rows, bool noflip, std::vector<G2P>& U,
                     std::vector<uint8_t>& flip, std::vector<uint8_t>& ok) {
  const size_t G = P.order.size();
  U.assign(G, proj_identity<Fp2>()); flip.assign(G, 0); ok.assign(G, 0);
  for (const KcLaunch& L : P.launches) {
    for (size_t i = L.lo; i < L.hi; ++i) {                 // k_kc_count
      const KcCom& k = cur.com[P.scom[i]];
      const KsCount c = kc_count(rows + P.srow[i], k.size, cbad.data() + k.wbase, noflip);
      flip[i] = c.flip; ok[i] = c.ok;
    }
    std::vector<int32_t> part(6 * NL * L.partials, 0);
    std::vector<uint8_t> written(L.partials, 0);
    for (size_t b = 0; b < L.n_items; ++b) {               // k_kc_word_sum, a workgroup per item
      const KcItem& it = P.items[L.item0 + b];
      const KcCom& k = cur.com[P.scom[it.first]];
      const uint32_t w = it.cword - k.wbase, left = kc_left(k.size, w);
      uint32_t mem[32];
      int32_t tile[KS_AFF_LIMBS * 32];
      for (uint32_t j = 0; j < 32; ++j) mem[j] = j < left ? cur_members[it.mbase + j] : 0;
      for (uint32_t t = 0; t < KS_AFF_LIMBS * 32; ++t) tile[t] = kc_tile_limb(aff.data(), n_keys, mem, left, t);
      for (uint32_t l = 0; l < it.count; ++l) {
        const size_t i = (size_t)it.first + l;
        const uint32_t m = ks_word_mask(ks_row_word(rows + P.srow[i], ks_row_bytes(k.size), w), flip[i] != 0, cskip[it.cword], ks_tail_mask(k.size, w));
        const size_t at = P.spbase[i] + w;
        if (at >= L.partials || written[at]) { std::fprintf(stderr, "partial %zu written twice or out of range\n", at); std::exit(3); }
        written[at] = 1;
        ks_store_point(part.data() + at, L.partials, ks_word_sum(m, tile));
      }
    }
    for (uint8_t v : written) if (!v) { std::fprintf(stderr, "a partial was not written\n"); std::exit(3); }
    std::vector<G2P> src(L.partials), dst;                 // the levels, as k_g2_seg_sum reads their descriptors
    for (size_t i = 0; i < L.partials; ++i) src[i] = ks_load_point(part.data() + i, L.partials);
    for (const SegLevel& lv : L.levels) {
      dst.assign(lv.count, proj_identity<Fp2>());
      for (size_t r = 0; r < lv.count; ++r)
        for (uint32_t j = 0; j < len[lv.first + r]; ++j) dst[r] = proj_add(dst[r], src[start[lv.first + r] + j]);
      src.swap(dst);
    }
    if (src.size() != L.hi - L.lo) { std::fprintf(stderr, "the levels do not end at one item per group\n"); std::exit(3); }
    for (size_t i = L.lo; i < L.hi; ++i) U[i] = src[i - L.lo];
  }
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s <command file>\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::string cmd;
  while (in >> cmd) {
    if (cmd == "set") {
      size_t n_keys, n_com; in >> n_keys >> n_com;
      const std::vector<uint64_t> off = nums<uint64_t>(in, n_com + 1);
      const std::vector<uint32_t> members = nums<uint32_t>(in, (size_t)off[n_com]);
      KcTable nw;
      std::string err = "-";
      const bool good = kc_build_table(members.data(), off.data(), n_com, n_keys, nw, err);
      if (good) { std::swap(cur, nw); cur_members = members; }
      for (char& ch : err) if (ch == ' ') ch = '_';
      std::printf("set %s %zu %s\n", good ? "ok" : "refused", cur.com.size(), err.c_str());
    } else if (cmd == "plan") {
      size_t chunk, ng; in >> chunk >> ng;
      const std::vector<uint32_t> com = nums<uint32_t>(in, ng);
      const std::vector<uint64_t> off = row_offsets(cur, com);
      KcPlan P;
      std::vector<uint32_t> start, len;
      if (!kc_plan(cur, com.data(), off.data(), ng, chunk, P, start, len)) return 3;
      std::printf("plan %zu %zu", P.launches.size(), P.items.size());
      for (uint32_t v : P.order) std::printf(" %u", v);
      for (uint32_t v : P.spbase) std::printf(" %u", v);
      for (uint64_t v : P.srow) std::printf(" %" PRIu64, v);
      for (const KcLaunch& L : P.launches) std::printf(" %zu %zu %zu %zu %zu %zu", L.lo, L.hi, L.item0, L.n_items, L.partials, L.levels.size());
      for (const KcItem& it : P.items) std::printf(" %u %u %u %u", it.cword, it.mbase, it.first, it.count);
      std::printf("\n");
    } else if (cmd == "words") {
      uint32_t n; in >> n;
      const std::vector<uint8_t> bad = blob(in), skip = blob(in), valid = blob(in);
      std::vector<uint32_t> cb, cs, cv;
      run_words(pack_words(bad, n).data(), pack_words(skip, n).data(), pack_words(valid, n).data(), cb, cs, cv);
      std::printf("words");
      for (const auto* v : {&cb, &cs, &cv}) for (uint32_t x : *v) std::printf(" %u", x);
      std::printf("\n");
    } else if (cmd == "count") {
      uint32_t size; int noflip; in >> size >> noflip;
      const std::vector<uint8_t> row = blob(in);
      const std::vector<uint32_t> cbad = nums<uint32_t>(in, ks_words(size));
      const KsCount c = kc_count(row.data(), size, cbad.data(), noflip != 0);
      std::printf("count %d %d\n", c.flip ? 1 : 0, c.ok ? 1 : 0);
    } else if (cmd == "rows") {
      size_t ng; in >> ng;
      const std::vector<uint32_t> com = nums<uint32_t>(in, ng);
      const std::vector<uint64_t> off = nums<uint64_t>(in, ng + 1);
      const std::vector<uint8_t> rows = blob(in);
      std::string err;
      const bool good = kc_check_rows(cur, com.data(), rows.data(), off.data(), ng, err);
      std::printf("rows %s\n", good ? "-1" : err.substr(6, err.find_first_of(": ", 6) - 6).c_str());
    } else if (cmd == "sum") {
      uint32_t n; size_t chunk, ng; in >> n >> chunk >> ng;
      const std::vector<uint32_t> com = nums<uint32_t>(in, ng);
      const std::vector<uint8_t> pks = blob(in), rows = blob(in);
      std::vector<int32_t> aff((size_t)KS_AFF_LIMBS * n);
      std::vector<uint32_t> bad(ks_words(n), 0), skip(ks_words(n), 0), cb, cs, cv;
      for (uint32_t i = 0; i < n; ++i) {                   // k_ks_register
        const KsKey k = ks_register(pks.data() + 128 * (size_t)i);
        ks_store_aff(aff.data() + i, n, k.p);
        if (k.bad) bad[i / 32] |= 1u << (i % 32);
        if (k.skip) skip[i / 32] |= 1u << (i % 32);
      }
      run_words(bad.data(), skip.data(), skip.data(), cb, cs, cv);
      // the totals: one all-ones row per committee, summed directly
      const size_t n_com = cur.com.size();
      std::vector<uint32_t> iota(n_com), start, len;
      std::vector<uint8_t> ones;
      for (size_t c = 0; c < n_com; ++c) {
        iota[c] = (uint32_t)c;
        const uint32_t size = cur.com[c].size;
        ones.insert(ones.end(), kc_row_bytes(size), 0xff);
        if (size & 7) ones.back() = (uint8_t)(0xffu >> (8 - (size & 7)));
      }
      KcPlan P;
      std::vector<G2P> T, U;
      std::vector<uint8_t> flip, ok;
      if (!kc_plan(cur, iota.data(), row_offsets(cur, iota).data(), n_com, chunk, P, start, len)) return 3;
      run_sums(P, start, len, aff, n, cb, cs, ones.data(), true, T, flip, ok);
      std::vector<int32_t> totals(6 * NL * n_com);
      for (size_t c = 0; c < n_com; ++c) ks_store_point(totals.data() + c, n_com, T[c]);      // sorted position = committee here
      // the call
      if (!kc_plan(cur, com.data(), row_offsets(cur, com).data(), ng, chunk, P, start, len)) return 3;
      run_sums(P, start, len, aff, n, cb, cs, rows.data(), false, U, flip, ok);
      std::vector<std::string> line(ng);
      for (size_t i = 0; i < ng; ++i) {                    // k_kc_finish and the encoding
        const G2P r = ks_finish(U[i], ks_load_point(totals.data() + P.scom[i], n_com), flip[i] != 0, ok[i] != 0);
        uint8_t enc[128];
        g2_encode(enc, g2_to_affine(r));
        char buf[300];
        int at = std::snprintf(buf, sizeof buf, " %d %d ", flip[i], ok[i]);
        for (int b = 0; b < 128; ++b) at += std::snprintf(buf + at, sizeof buf - at, "%02x", enc[b]);
        line[P.order[i]] = buf;
      }
      std::printf("sum");
      for (const std::string& s : line) std::printf("%s", s.c_str());
      std::printf(" %zu\n", P.launches.size());
    } else { std::fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
  }
  return 0;
}
