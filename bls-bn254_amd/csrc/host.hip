// host.hip -- C-ABI host side (include/blsbn254.h), core unit: contexts, profiling, the VALU probe, staging helpers, the final-
// exponentiation pipeline, and the primitive entry points (pairing, Miller loop, hash to curve, point checks).
// The other pipelines: host_verify.hip (verify + G2Prepared), host_rlc.hip (RLC batch verification), host_aggregate.hip
// (aggregate verify, sums, threshold), host_groupops.hip (group operations, FastAggregateVerify), host_pairing_check.hip
// (pairing-product equations over groups of pairs), host_misc.hip.
#include "host_common.h"
#include "lane_hash_tai.h"   // the map ids (G1MAP_*) the header's are checked against

extern "C" {

// -G2gen = (x, p - y) of the generator fp2.rs:305-333, as bytes
const uint8_t NEG_G2_BYTES[128] = {
  0x19,0x8e,0x93,0x93,0x92,0x0d,0x48,0x3a,0x72,0x60,0xbf,0xb7,0x31,0xfb,0x5d,0x25,0xf1,0xaa,0x49,0x33,0x35,0xa9,0xe7,0x12,0x97,0xe4,0x85,0xb7,0xae,0xf3,0x12,0xc2,
  0x18,0x00,0xde,0xef,0x12,0x1f,0x1e,0x76,0x42,0x6a,0x00,0x66,0x5e,0x5c,0x44,0x79,0x67,0x43,0x22,0xd4,0xf7,0x5e,0xda,0xdd,0x46,0xde,0xbd,0x5c,0xd9,0x92,0xf6,0xed,
  0x27,0x5d,0xc4,0xa2,0x88,0xd1,0xaf,0xb3,0xcb,0xb1,0xac,0x09,0x18,0x75,0x24,0xc7,0xdb,0x36,0x39,0x5d,0xf7,0xbe,0x3b,0x99,0xe6,0x73,0xb1,0x3a,0x07,0x5a,0x65,0xec,
  0x1d,0x9b,0xef,0xcd,0x05,0xa5,0x32,0x3e,0x6d,0xa4,0xd4,0x35,0xf3,0xb6,0x17,0xcd,0xb3,0xaf,0x83,0x28,0x5c,0x2d,0xf7,0x11,0xef,0x39,0xc0,0x15,0x71,0x82,0x7f,0x9d};


const char* blsbn254_strerror(int code) {
  switch (code) {
    case 0: return "ok";
    case 1: return "invalid scalar bytes";
    case 2: return "invalid G1 bytes";
    case 3: return "invalid G2 bytes";
    case 4: return "invalid Gt bytes";
    case BLSBN254_ST_SHORT: return "too few usable partial signatures";
    case BLSBN254_E_ARG: return "invalid argument";
    case BLSBN254_E_HIP: return "HIP runtime error";
    case BLSBN254_E_NOMEM: return "out of device memory";
    case BLSBN254_E_NO_DEVICE: return "no gfx950 device available (there is no CPU fallback)";
    case BLSBN254_E_RCCL: return "RCCL error";
    default: return "unknown error";
  }
}
const char* blsbn254_last_error(blsbn254_ctx* ctx) { return ctx ? ctx->last_error.c_str() : ""; }

int blsbn254_ctx_create(int device, blsbn254_ctx** out) {
  if (!out) return BLSBN254_E_ARG;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return BLSBN254_E_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return BLSBN254_E_NO_DEVICE;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return BLSBN254_E_NO_DEVICE;
  blsbn254_ctx* c = new blsbn254_ctx();
  c->device = device;
  if (const char* e = std::getenv("BLSBN254_CHUNK_LANES")) {
    size_t v = (size_t)std::strtoull(e, nullptr, 10) & ~(size_t)7;        // multiples of 8: bitmap bytes must not straddle chunks
    if (v >= 8 && v <= ((size_t)1 << 23)) c->chunk = v;
  }
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return BLSBN254_E_HIP; }
  if (hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) { (void)hipStreamDestroy(c->stream); delete c; return BLSBN254_E_HIP; }
  if (getrandom(&c->kd.seed, sizeof c->kd.seed, 0) != (ssize_t)sizeof c->kd.seed) c->kd.seed = 0x5bd1e995u;
  c->forms = forms_from_env([](const char* name) -> const char* { return std::getenv(name); }, prop.multiProcessorCount);
  if (const char* e = std::getenv("BLSBN254_AUTO_PREPARE")) c->auto_prepare = std::atoi(e) != 0;
  if (const char* e = std::getenv("BLSBN254_RLC_GROUP")) { long v = std::atol(e); if (v >= 2 && v <= (long)RLC_MAX_GROUP) { c->r2.group = (size_t)v; c->r2.group_auto = false; } }
  if (const char* e = std::getenv("BLSBN254_RLC_KEY_ROUND")) c->r2.key_round = std::atoi(e) != 0;
  if (const char* e = std::getenv("BLSBN254_ASYNC_VERIFY")) c->vq.async = std::atoi(e) != 0;
  if (const char* e = std::getenv("BLSBN254_KEY_CACHE")) { long v = std::atol(e); if (v >= 0 && v <= (long)PREP_MAX_KEYS) c->kc.max = (size_t)v; }
  *out = c;
  return 0;
}
void blsbn254_ctx_destroy(blsbn254_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);               // nothing is freed while either stream may still run work that touches it
  (void)hipStreamSynchronize(c->stream2);
  for (auto& pv : c->vq.pend) if (pv.ev) (void)hipEventDestroy(pv.ev);       // pending checks are dropped: the caller did not ask for their results
  if (c->vq.host) (void)hipHostFree(c->vq.host);
  for (auto& kv : c->prof) for (auto& pr : kv.second.pending) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
  (void)hipEventDestroy(c->ev_fork); (void)hipEventDestroy(c->ev_join);
  (void)hipStreamDestroy(c->stream2);
  (void)hipStreamDestroy(c->stream);
  delete c;                                            // every DevBuf frees itself
}
int blsbn254_ctx_synchronize(blsbn254_ctx* c) {
  if (!c) return BLSBN254_E_ARG;
  ENTER(c);                                           // settles the asynchronously enqueued verify calls (re-running one whose assumption failed)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
void* blsbn254_ctx_stream(blsbn254_ctx* c) { return c ? (void*)c->stream : nullptr; }

int blsbn254_profile_enable(blsbn254_ctx* c, int on) { if (!c) return BLSBN254_E_ARG; c->profiling = on != 0; return 0; }
int blsbn254_profile_reset(blsbn254_ctx* c) {
  if (!c) return BLSBN254_E_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (auto& kv : c->prof) for (auto& pr : kv.second.pending) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
  c->prof.clear();
  return 0;
}
int blsbn254_profile_read(blsbn254_ctx* c, char* names, uint64_t* launches, double* total_ms, int max_entries) {
  if (!c) return BLSBN254_E_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int k = 0;
  for (auto& kv : c->prof) {
    ProfEntry& p = kv.second;
    for (auto& pr : p.pending) { float ms = 0; (void)hipEventElapsedTime(&ms, pr.first, pr.second); p.ms += ms; (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    p.pending.clear();
    if (k < max_entries) { std::snprintf(names + 32 * k, 32, "%s", kv.first.c_str()); launches[k] = p.launches; total_ms[k] = p.ms; ++k; }
  }
  return k;
}

// VALU roofline probe (k_valu_peak, k_misc.hip), 4 waves per SIMD on every CU:
//   out[0] v_mad_u64_u32 lane-MADs per second          out[1] plain VOP2 (v_add_u32 / v_xor_b32) lane-ops per second
//   out[2] shader clock held under the MAD probe (Hz)  out[3] shader clock held under the VOP2 probe (Hz)
//   out[4] compute units                               out[5] 4-cycle issue ceiling = CUs x 4 SIMDs x 16 lane-ops/cycle x out[2]
//   (what ONE wave per SIMD can issue: a wave64 VALU instruction every 4 cycles; with several waves per SIMD plain VOP2
//   work issues faster than that -- out[1] -- while v_mad_u64_u32 does not -- out[0])
// The clock is delta(s_memtime) / delta(s_memrealtime) x 100 MHz, median over all waves (MI355X_MICROARCH.md, DVFS item 6).
struct EventPair {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~EventPair() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};
int blsbn254_valu_probe(blsbn254_ctx* c, double out[6]) {
  if (!c || !out) return BLSBN254_E_ARG;
  ENTER(c);
  hipDeviceProp_t prop;
  HIPCHK(c, hipGetDeviceProperties(&prop, c->device));
  const int blocks = prop.multiProcessorCount * 4, iters = 1 << 16;
  const size_t nwaves = (size_t)blocks * 4;
  HIPCHK(c, c->misc.reserve((size_t)blocks * 256 * 4 + 64 + nwaves * 16));
  uint64_t* d_stamps = (uint64_t*)((char*)c->misc.p + (((size_t)blocks * 256 * 4 + 63) & ~(size_t)63));
  EventPair ev;                                   // destroyed on every return path
  HIPCHK(c, hipEventCreate(&ev.e0)); HIPCHK(c, hipEventCreate(&ev.e1));
  std::vector<uint64_t> st(nwaves * 2);
  std::vector<double> clk(nwaves);
  for (int kind = 0; kind < 2; ++kind) {
    double best = 0, best_clk = 0;
    for (int rep = 0; rep < 4; ++rep) {
      HIPCHK(c, hipEventRecord(ev.e0, c->stream));
      TRY(launch(c, c->stream, nullptr, Shape{dim3(blocks), dim3(256)}, k_valu_peak, (uint32_t*)c->misc.p, 1u + rep, iters, kind, d_stamps));
      HIPCHK(c, hipEventRecord(ev.e1, c->stream));
      HIPCHK(c, hipEventSynchronize(ev.e1));
      float ms = 0; HIPCHK(c, hipEventElapsedTime(&ms, ev.e0, ev.e1));
      double rate = (double)blocks * 256 * iters * 8 / (ms * 1e-3);
      if (rep > 0 && rate > best) {                    // rep 0 warms the clocks
        best = rate;
        HIPCHK(c, hipMemcpy(st.data(), d_stamps, nwaves * 16, hipMemcpyDeviceToHost));
        for (size_t w = 0; w < nwaves; ++w) clk[w] = st[2 * w + 1] ? (double)st[2 * w] / (double)st[2 * w + 1] * 100e6 : 0;
        std::nth_element(clk.begin(), clk.begin() + nwaves / 2, clk.end());
        best_clk = clk[nwaves / 2];
      }
    }
    out[kind] = best; out[2 + kind] = best_clk;
  }
  out[4] = prop.multiProcessorCount;
  out[5] = (double)prop.multiProcessorCount * 4.0 * 16.0 * out[2];   // one wave64 instruction per 4 cycles per SIMD = 16 lane-ops per cycle per SIMD
  return 0;
}
// Measured v_mad_u64_u32 issue rate of the whole chip (lane-MADs per second): out[0] of the probe above.
int blsbn254_valu_peak(blsbn254_ctx* c, double* mads_per_s) {
  if (!c || !mads_per_s) return BLSBN254_E_ARG;
  double o[6];
  int rc = blsbn254_valu_probe(c, o);
  if (rc) return rc;
  *mads_per_s = o[0];
  return 0;
}

// The message expander of every hashing launch (host_common.h launch_hash_to_g1 and its siblings).  Settles the context FIRST: a
// pending asynchronous verify call whose guess fails is re-run by resolve_pending from its saved DST, and that re-run must hash under
// the expander the call was made with -- so the pending calls are resolved (ENTER) before the new id is stored.  The resident
// tag is dropped: the staged bytes of an oversize DST depend on the expander.
static_assert(BLSBN254_EXPAND_XMD_SHA256 == EXPAND_XMD_SHA256 && BLSBN254_EXPAND_XMD_KECCAK256 == EXPAND_XMD_KECCAK256 && BLSBN254_EXPAND_XMD_SHA3_256 == EXPAND_XMD_SHA3_256 &&
              BLSBN254_EXPAND_XOF_SHAKE128 == EXPAND_XOF_SHAKE128 && BLSBN254_EXPAND_XOF_SHAKE256 == EXPAND_XOF_SHAKE256, "the header's ids are keccak.h's");
int blsbn254_set_expander(blsbn254_ctx* c, int id) {
  if (!c || id < 0 || id >= (int)EXPAND_COUNT) return BLSBN254_E_ARG;
  ENTER(c);
  c->expander = (uint32_t)id;
  c->dst_host_len = -1;
  return 0;
}
int blsbn254_get_expander(const blsbn254_ctx* c) { return c ? (int)c->expander : BLSBN254_E_ARG; }

// The map behind every message hashed to G1 (host_common.h launch_hash_to_g1 / launch_sign).  Settles the context FIRST, as
// blsbn254_set_expander does and for the same reason: a pending asynchronous verify call whose guess fails is re-run by
// resolve_pending, and that re-run must hash under the map the call was made with.  The resident tag stays: no map changes it.
static_assert(BLSBN254_G1MAP_SVDW == G1MAP_SVDW && BLSBN254_G1MAP_TAI_DIGEST == G1MAP_TAI_DIGEST && BLSBN254_G1MAP_TAI_HASH == G1MAP_TAI_HASH,
              "the header's ids are lane_hash_tai.h's");
int blsbn254_set_g1_map(blsbn254_ctx* c, int id) {
  if (!c || id < 0 || id >= (int)G1MAP_COUNT) return BLSBN254_E_ARG;
  ENTER(c);
  c->g1_map = (uint32_t)id;
  return 0;
}
int blsbn254_get_g1_map(const blsbn254_ctx* c) { return c ? (int)c->g1_map : BLSBN254_E_ARG; }

// DST handling: RFC 9380 5.3.3 (an oversize DST is pre-hashed with the context's expander, keccak.h oversize_dst); staged into
// device memory once per call
int stage_dst(blsbn254_ctx* c, const uint8_t* dst, size_t dst_len, uint32_t* out_len) {
  uint8_t tmp[256];
  if (dst_len > 255) {
    oversize_dst(c->expander, tmp, dst, dst_len);
    dst_len = 32;
  } else if (dst_len) std::memcpy(tmp, dst, dst_len);
  *out_len = (uint32_t)dst_len;
  // the same tag as the previous call (every step of a steady-state caller): already resident, nothing to copy or wait for
  if (c->dst_host_len == (int)dst_len && (dst_len == 0 || std::memcmp(c->dst_host, tmp, dst_len) == 0)) return 0;
  HIPCHK(c, c->dst.reserve(256));
  c->dst_host_len = -1;
  if (dst_len) {
    HIPCHK(c, hipStreamSynchronize(c->stream));           // kernels of an earlier call may still be reading the old tag
    std::memcpy(c->dst_host, tmp, dst_len);                // ctx-owned source: outlives the asynchronous copy
    HIPCHK(c, hipMemcpyAsync(c->dst.p, c->dst_host, dst_len, hipMemcpyHostToDevice, c->stream));
  }
  c->dst_host_len = (int)dst_len;
  return 0;
}
int check_offsets(const uint64_t* off, size_t n) {
  for (size_t i = 0; i < n; ++i) if (off[i + 1] < off[i]) return BLSBN254_E_ARG;
  return 0;
}
int min_index_arm(blsbn254_ctx* c, int* d, size_t words) {
  static const int none[2] = {NO_INDEX, NO_INDEX};          // static: outlives the asynchronous copy
  HIPCHK(c, hipMemcpyAsync(d, none, 4 * words, hipMemcpyHostToDevice, c->stream));
  return 0;
}
int min_index_read(blsbn254_ctx* c, const int* d, int* out) {
  TRY(download(c, out, d, 4));
  if (*out == NO_INDEX) *out = -1;
  return 0;
}
// first index whose status differs from the wanted value, or -1
int first_bad(blsbn254_ctx* c, const uint8_t* d_status, size_t n, uint8_t mask, uint8_t val, int* out) {
  HIPCHK(c, c->misc.reserve(64));
  TRY(min_index_arm(c, (int*)c->misc.p, 1));
  TRY(launch(c, c->stream, "status_reduce", grid_lanes(n), k_status_reduce, d_status, n, mask, val, (int*)c->misc.p));
  return min_index_read(c, (const int*)c->misc.p, out);
}
// status byte of the tuple at index idx (host read)
int read_status(blsbn254_ctx* c, const uint8_t* d_status, int idx, uint8_t* st) { return download(c, st, d_status + idx, 1); }


// Final exponentiation of the n Fp12 values at f (limb-major, `stride`), in place for the easy part.
//   mode 0: verify bitmap (flags / sub_ok / d_bitmap)   mode 1: Gt bytes   mode 3: single is_one flag (n == 1)
int run_final_exp(blsbn254_ctx* c, int32_t* f, size_t n, size_t stride, int mode, const uint8_t* flags, const uint8_t* sub_ok,
                         uint8_t* d_bitmap, uint8_t* d_gt, int* d_is_one) {
  CHECK_LANES(c, stride);
  for (DevBuf& b : c->fe.ph) HIPCHK(c, b.reserve(stride * 108 * 4));
  HIPCHK(c, c->fe.slots.reserve(stride * 108 * 4 * 10));
  int32_t* S = (int32_t*)c->fe.slots.p;
  int32_t *X = (int32_t*)c->fe.ph[0].p, *A = (int32_t*)c->fe.ph[1].p, *B = (int32_t*)c->fe.ph[2].p, *C = (int32_t*)c->fe.ph[3].p,
          *B2 = (int32_t*)c->fe.ph[4].p, *D = (int32_t*)c->fe.ph[5].p;
  // t = f^((p^6-1)(p^2+1)), in place (split: the pieces wait in the phase buffers A and B, which the hard part only fills later)
  if (fe_easy_split(c->forms, n)) {
    TRY(launch(c, c->stream, "fe_easy_head", grid_lanes(n), k_fe_easy_head, (const int32_t*)f, n, stride, A, B));
    TRY(launch(c, c->stream, "fe_inv4", grid_lanes((n + 3) / 4), k_fe_inv4, B, n, stride));
    TRY(launch(c, c->stream, "fe_easy_tail", grid_lanes(n), k_fe_easy_tail, (const int32_t*)f, f, n, stride, (const int32_t*)A, (const int32_t*)B));
  } else {
    TRY(launch(c, c->stream, "fe_easy", grid_lanes(n), k_fe_easy, (const int32_t*)f, f, n, stride));
  }
  // the hard part: the wave and quad forms leave a validity byte per tuple (mode 0), packed behind them
  const Form form = fe_hard_form(c->forms, n);
  if (form != Form::LANE) {
    uint8_t* one = nullptr;
    if (form == Form::TRI) HIPCHK(c, c->fe.tri.reserve(n * TRI_VALUE_LIMBS * 4));
    if (mode == 0) { HIPCHK(c, c->fe.one.reserve(n)); one = (uint8_t*)c->fe.one.p; }
    if (form == Form::WIDE) TRY(launch(c, c->stream, "fe_hard_wide", grid_wide(n), k_fe_hard_wide, (const int32_t*)f, n, stride, flags, sub_ok, one, d_gt, d_is_one, mode));
    else TRY(launch(c, c->stream, "fe_tri_hard", grid_tri(n), k_fe_tri_hard, (const int32_t*)f, n, stride, (int32_t*)c->fe.tri.p, flags, sub_ok, one, d_gt, d_is_one, mode));
    if (mode == 0) TRY(launch(c, c->stream, "pack_bitmap", grid_lanes(n), k_pack_bitmap, (const uint8_t*)one, n, d_bitmap));
    return 0;
  }
  // t^x three times; the glue steps fe_h1 / fe_h2 are computed by the first two launches themselves (k_fe_expx_tail.hip)
  TRY(launch(c, c->stream, "fe_expx_h1", grid_lanes(n), k_fe_expx_h1, (const int32_t*)f, S, n, stride, A, B));
  TRY(launch(c, c->stream, "fe_expx_h2", grid_lanes(n), k_fe_expx_h2, (const int32_t*)B, S, n, stride, B, C, B2, D));
  TRY(launch(c, c->stream, "fe_expx", grid_lanes(n), k_fe_expx, (const int32_t*)D, X, S, n, stride));
  TRY(launch(c, c->stream, "fe_h3", grid_lanes(n), k_fe_h3, (const int32_t*)f, (const int32_t*)A, (const int32_t*)C, (const int32_t*)B2, (const int32_t*)X, S, n, stride,
             flags, sub_ok, d_bitmap, d_gt, d_is_one, mode));
  return 0;
}

// ---------------- pairing / Miller loop / final exponentiation
int miller_to_ws(blsbn254_ctx* c, const uint8_t* d_g1, const uint8_t* d_g2, size_t n) {
  CHECK_LANES(c, n);
  HIPCHK(c, c->f_ws.reserve(n * 108 * 4));
  HIPCHK(c, c->status.reserve(n));
  int32_t* f = (int32_t*)c->f_ws.p; uint8_t* st = (uint8_t*)c->status.p;
  switch (miller_form(c->forms, n)) {
    case Form::WIDE: return launch(c, c->stream, "miller_wide_1", grid_wide(n), k_miller_wide_1, d_g1, d_g2, n, f, n, st);
    case Form::TRI: return launch(c, c->stream, "miller_tri_1", grid_tri(n), k_miller_tri_1, d_g1, d_g2, n, f, n, st);
    case Form::LANE: break;
  }
  return launch(c, c->stream, "miller_1", grid_lanes(n), k_miller_1, d_g1, d_g2, n, f, n, st);
}
int decode_status_rc(blsbn254_ctx* c, const uint8_t* d_status, size_t n) {
  int bad;
  int rc = first_bad(c, d_status, n, 3, 3, &bad);
  if (rc) return rc;
  if (bad < 0) return 0;
  uint8_t st; rc = read_status(c, d_status, bad, &st);
  if (rc) return rc;
  return (st & 1) ? BLSBN254_ERR_G2 : BLSBN254_ERR_G1;
}
int blsbn254_pairing_batch_dev(blsbn254_ctx* c, const uint8_t* d_g1, const uint8_t* d_g2, size_t n, uint8_t* d_gt, uint8_t* d_status) {
  if (!c || (n && (!d_g1 || !d_g2 || !d_gt))) return BLSBN254_E_ARG;
  if (n == 0) return 0;
  ENTER(c);
  HIPCHK(c, c->status_all.reserve(n));
  TRY(for_chunks(c, n, [&](size_t lo, size_t m) -> int {
    TRY(miller_to_ws(c, d_g1 + 64 * lo, d_g2 + 128 * lo, m));
    TRY(run_final_exp(c, (int32_t*)c->f_ws.p, m, m, 1, nullptr, nullptr, nullptr, d_gt + 384 * lo, nullptr));
    HIPCHK(c, hipMemcpyAsync((uint8_t*)c->status_all.p + lo, c->status.p, m, hipMemcpyDeviceToDevice, c->stream));
    return 0;
  }));
  if (d_status) HIPCHK(c, hipMemcpyAsync(d_status, c->status_all.p, n, hipMemcpyDeviceToDevice, c->stream));
  return 0;
}
int blsbn254_pairing_batch(blsbn254_ctx* c, const uint8_t* g1, const uint8_t* g2, size_t n, uint8_t* gt) {
  if (!c || (n && (!g1 || !g2 || !gt))) return BLSBN254_E_ARG;
  if (n == 0) return 0;
  ENTER(c);
  HIPCHK(c, c->out.reserve(384 * n));
  TRY(upload(c, c->in_a, g1, 64 * n));
  TRY(upload(c, c->in_b, g2, 128 * n));
  int rc = blsbn254_pairing_batch_dev(c, (const uint8_t*)c->in_a.p, (const uint8_t*)c->in_b.p, n, (uint8_t*)c->out.p, nullptr);
  if (rc) return rc;
  rc = decode_status_rc(c, (const uint8_t*)c->status_all.p, n);
  if (rc) return rc;
  return download(c, gt, c->out.p, 384 * n);
}
int blsbn254_miller_loop_batch(blsbn254_ctx* c, const uint8_t* g1, const uint8_t* g2, size_t n, uint8_t* ml_out) {
  if (!c || (n && (!g1 || !g2 || !ml_out))) return BLSBN254_E_ARG;
  if (n == 0) return 0;
  ENTER(c);
  HIPCHK(c, c->out.reserve(384 * n));
  TRY(upload(c, c->in_a, g1, 64 * n));
  TRY(upload(c, c->in_b, g2, 128 * n));
  TRY(for_chunks(c, n, [&](size_t lo, size_t m) -> int {
    TRY(miller_to_ws(c, (const uint8_t*)c->in_a.p + 64 * lo, (const uint8_t*)c->in_b.p + 128 * lo, m));
    TRY(decode_status_rc(c, (const uint8_t*)c->status.p, m));
    return launch(c, c->stream, "fp12_to_bytes", grid_lanes(m), k_fp12_to_bytes, (const int32_t*)c->f_ws.p, m, m, (uint8_t*)c->out.p + 384 * lo);
  }));
  return download(c, ml_out, c->out.p, 384 * n);
}
int blsbn254_multi_miller_loop(blsbn254_ctx* c, const uint8_t* g1, const uint8_t* g2, size_t n, uint8_t ml_out[384]) {
  if (!c || !ml_out || (n && (!g1 || !g2))) return BLSBN254_E_ARG;
  if (n == 0) { std::memset(ml_out, 0, 384); ml_out[31] = 1; return 0; }       // empty product = Fp12::ONE
  CHECK_LANES(c, n);
  ENTER(c);
  HIPCHK(c, c->out.reserve(384));
  TRY(upload(c, c->in_a, g1, 64 * n));
  TRY(upload(c, c->in_b, g2, 128 * n));
  int rc = miller_to_ws(c, (const uint8_t*)c->in_a.p, (const uint8_t*)c->in_b.p, n);
  if (rc) return rc;
  rc = decode_status_rc(c, (const uint8_t*)c->status.p, n);
  if (rc) return rc;
  int32_t* res; size_t rs;
  rc = fp12_tree(c, (int32_t*)c->f_ws.p, n, n, &res, &rs);
  if (rc) return rc;
  TRY(launch(c, c->stream, "fp12_to_bytes", grid_lanes(1), k_fp12_to_bytes, (const int32_t*)res, (size_t)1, rs, (uint8_t*)c->out.p));
  return download(c, ml_out, c->out.p, 384);
}
int blsbn254_final_exponentiation(blsbn254_ctx* c, const uint8_t* ml, size_t n, uint8_t* gt) {
  if (!c || (n && (!ml || !gt))) return BLSBN254_E_ARG;
  if (n == 0) return 0;
  ENTER(c);
  HIPCHK(c, c->out.reserve(384 * n));
  TRY(upload(c, c->in_a, ml, 384 * n));
  TRY(for_chunks(c, n, [&](size_t lo, size_t m) -> int {
    HIPCHK(c, c->f_ws.reserve(m * 108 * 4)); HIPCHK(c, c->status.reserve(m));
    TRY(launch(c, c->stream, "fp12_from_bytes", grid_lanes(m), k_fp12_from_bytes, (const uint8_t*)c->in_a.p + 384 * lo, m, (int32_t*)c->f_ws.p, m, (uint8_t*)c->status.p));
    int bad;
    TRY(first_bad(c, (const uint8_t*)c->status.p, m, 1, 1, &bad));
    if (bad >= 0) return BLSBN254_ERR_GT;
    return run_final_exp(c, (int32_t*)c->f_ws.p, m, m, 1, nullptr, nullptr, nullptr, (uint8_t*)c->out.p + 384 * lo, nullptr);
  }));
  return download(c, gt, c->out.p, 384 * n);
}

// ---------------- hash to curve
int stage_msgs(blsbn254_ctx* c, const uint8_t* msgs, const uint64_t* off, size_t n) {
  if (check_offsets(off, n)) return BLSBN254_E_ARG;
  size_t total = (size_t)(off[n] - off[0]);
  HIPCHK(c, c->in_c.reserve(total + 1)); HIPCHK(c, c->in_off.reserve(8 * (n + 1)));
  if (total) HIPCHK(c, hipMemcpyAsync(c->in_c.p, msgs + off[0], total, hipMemcpyHostToDevice, c->stream));
  if (off[0] == 0) HIPCHK(c, hipMemcpyAsync(c->in_off.p, off, 8 * (n + 1), hipMemcpyHostToDevice, c->stream));
  else {
    std::vector<uint64_t> rel(n + 1);
    for (size_t i = 0; i <= n; ++i) rel[i] = off[i] - off[0];
    HIPCHK(c, hipMemcpyAsync(c->in_off.p, rel.data(), 8 * (n + 1), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return 0;
}
static int h2c_common(blsbn254_ctx* c, const uint8_t* msgs, const uint64_t* off, size_t n, const uint8_t* dst, size_t dst_len, uint8_t* out, int g2, int ro) {
  if (!c || (n && (!msgs && off && off[n] != off[0])) || !off || (n && !out) || (dst_len && !dst)) return BLSBN254_E_ARG;
  if (n == 0) return 0;
  ENTER(c);
  uint32_t dl; int rc = stage_dst(c, dst, dst_len, &dl);
  if (rc) return rc;
  rc = stage_msgs(c, msgs, off, n);
  if (rc) return rc;
  size_t sz = g2 ? 128 : 64;
  HIPCHK(c, c->out.reserve(sz * n));
  if (g2) TRY(launch_hash_to_g2(c, c->stream, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, n, dl, (uint8_t*)c->out.p, ro));
  else TRY(launch_hash_to_g1(c, c->stream, (const uint8_t*)c->in_c.p, (const uint64_t*)c->in_off.p, n, dl, (int32_t*)nullptr,
                  n, (uint8_t*)c->out.p, ro ? 1 : 2));
  return download(c, out, c->out.p, sz * n);
}
int blsbn254_hash_to_g1_batch(blsbn254_ctx* c, const uint8_t* m, const uint64_t* o, size_t n, const uint8_t* d, size_t dl, uint8_t* out) { return h2c_common(c, m, o, n, d, dl, out, 0, 1); }
int blsbn254_encode_to_g1_batch(blsbn254_ctx* c, const uint8_t* m, const uint64_t* o, size_t n, const uint8_t* d, size_t dl, uint8_t* out) { return h2c_common(c, m, o, n, d, dl, out, 0, 0); }
int blsbn254_hash_to_g2_batch(blsbn254_ctx* c, const uint8_t* m, const uint64_t* o, size_t n, const uint8_t* d, size_t dl, uint8_t* out) { return h2c_common(c, m, o, n, d, dl, out, 1, 1); }
int blsbn254_encode_to_g2_batch(blsbn254_ctx* c, const uint8_t* m, const uint64_t* o, size_t n, const uint8_t* d, size_t dl, uint8_t* out) { return h2c_common(c, m, o, n, d, dl, out, 1, 0); }

// ---------------- point checks
static int check_common(blsbn254_ctx* c, const uint8_t* pts, size_t n, uint8_t* bm, int g2) {
  if (!c || (n && (!pts || !bm))) return BLSBN254_E_ARG;
  if (n == 0) return 0;
  ENTER(c);
  size_t sz = g2 ? 128 : 64, nb = (n + 7) / 8;
  HIPCHK(c, c->bitmap.reserve(nb + 8));
  TRY(upload(c, c->in_a, pts, sz * n));
  if (g2) TRY(launch(c, c->stream, "g2_check", grid_lanes(n), k_g2_check, (const uint8_t*)c->in_a.p, n, (uint8_t*)nullptr, (uint8_t*)c->bitmap.p));
  else TRY(launch(c, c->stream, "g1_check", grid_lanes(n), k_g1_check, (const uint8_t*)c->in_a.p, n, (uint8_t*)c->bitmap.p));
  return download(c, bm, c->bitmap.p, nb);
}
int blsbn254_g1_check_batch(blsbn254_ctx* c, const uint8_t* g1, size_t n, uint8_t* bm) { return check_common(c, g1, n, bm, 0); }
int blsbn254_g2_check_batch(blsbn254_ctx* c, const uint8_t* g2, size_t n, uint8_t* bm) { return check_common(c, g2, n, bm, 1); }


}  // extern "C"
