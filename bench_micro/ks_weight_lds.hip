// Stake weights by bitmap (k_ks_weight, csrc/k_keyset_weight.hip): the table read from global memory (L2-resident) against the
// table staged in LDS.  Both forms run the product's lane function (kw_lane_sum, csrc/keyset_weight.h) and its wave reduction,
// a wave per group; they differ only in where `eff` points.
//   global   the product's kernel: four groups per workgroup, every selected key read through L1 / L2
//   lds      a workgroup stages the WHOLE table (8 n_keys n_cols bytes, at most 64 KB) into LDS once, then each of its four
//            waves weighs GPW groups out of it -- the staging is paid once per 4 GPW groups (GPW = 1: the product's layout)
// 4096 groups over 1024 keys at 2/3 participation, 1 and 4 columns: median of 20 timed launches after 3 warm-ups, HIP events;
// the two forms' outputs are compared.  DESIGN.md 6k records the figures and the decision.
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 bench_micro/ks_weight_lds.hip -o bench_micro/ks_weight_lds
#include "../bls-bn254_amd/csrc/keyset_weight.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
using namespace bn;
#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

__device__ inline void wave_store(KwAcc a, uint32_t lane, uint32_t n_cols, uint64_t* out) {
#pragma unroll
  for (uint32_t d = KW_WAVE / 2; d; d >>= 1) {
#pragma unroll
    for (uint32_t q = 0; q < KW_COLS; ++q)
      if (q < n_cols) {
        const uint32_t lo = (uint32_t)__shfl_down((int)kw_lo(a.v[q]), d), hi = (uint32_t)__shfl_down((int)kw_hi(a.v[q]), d);
        a.v[q] += kw_join(lo, hi);
      }
  }
  if (lane == 0) {
#pragma unroll
    for (uint32_t q = 0; q < KW_COLS; ++q)
      if (q < n_cols) out[q] = a.v[q];
  }
}
__global__ void __launch_bounds__(256) k_global(const uint8_t* rows, const uint32_t* vwords, const uint64_t* eff, uint32_t n_keys, uint32_t n_cols, size_t m, uint64_t* out) {
  const size_t g = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (g >= m) return;
  const uint32_t lane = threadIdx.x & 63;
  wave_store(kw_lane_sum(rows + g * ks_row_bytes(n_keys), n_keys, lane, vwords, eff, n_cols), lane, n_cols, out + g * n_cols);
}
template <int GPW>
__global__ void __launch_bounds__(256) k_lds(const uint8_t* rows, const uint32_t* vwords, const uint64_t* eff, uint32_t n_keys, uint32_t n_cols, size_t m, uint64_t* out) {
  extern __shared__ uint64_t tile[];
  for (uint32_t t = threadIdx.x; t < n_keys * n_cols; t += blockDim.x) tile[t] = eff[t];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 1
  for (int r = 0; r < GPW; ++r) {
    const size_t g = ((size_t)blockIdx.x * 4 + wave) * GPW + r;
    if (g >= m) return;                                    // the whole wave, behind the only barrier
    wave_store(kw_lane_sum(rows + g * ks_row_bytes(n_keys), n_keys, lane, vwords, tile, n_cols), lane, n_cols, out + g * n_cols);
  }
}

static float median_ms(std::vector<float>& v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main() {
  const uint32_t n = 1024; const size_t G = 4096, rb = (n + 7) / 8;
  std::vector<uint8_t> rows(G * rb);
  uint64_t s = 88172645463325252ull;
  auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
  for (size_t g = 0; g < G; ++g)
    for (uint32_t i = 0; i < n; ++i)
      if (rnd() % 3 != 0) rows[g * rb + (i >> 3)] |= (uint8_t)(1u << (i & 7));
  uint8_t* d_rows; uint64_t *d_eff, *d_out[2]; uint32_t* d_vw;
  CHK(hipMalloc(&d_vw, 4 * (n / 32))); CHK(hipMemset(d_vw, 0xff, 4 * (n / 32)));      // every key valid
  CHK(hipMalloc(&d_rows, rows.size())); CHK(hipMemcpy(d_rows, rows.data(), rows.size(), hipMemcpyHostToDevice));
  CHK(hipMalloc(&d_eff, 8 * n * KW_COLS)); CHK(hipMalloc(&d_out[0], 8 * G * KW_COLS)); CHK(hipMalloc(&d_out[1], 8 * G * KW_COLS));
  hipEvent_t e0, e1; CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
  printf("{\"ks_weight_lds\": {\"groups\": %zu, \"keys\": %u, \"participation\": \"2/3\", \"rows\": [\n", G, n);
  bool first = true;
  for (uint32_t nc : {1u, 4u}) {
    std::vector<uint64_t> eff((size_t)n * nc), ref(G * nc);
    for (auto& v : eff) v = rnd() >> 24;
    CHK(hipMemcpy(d_eff, eff.data(), 8 * eff.size(), hipMemcpyHostToDevice));
    const size_t lds = 8 * (size_t)n * nc;
    for (int form = 0; form < 4; ++form) {                 // 0: global; 1..3: lds with 1, 4, 16 groups per wave
      const int gpw = form == 0 ? 1 : form == 1 ? 1 : form == 2 ? 4 : 16;
      const unsigned blocks = (unsigned)((G + 4 * gpw - 1) / (4 * gpw));
      uint64_t* o = d_out[form ? 1 : 0];
      std::vector<float> ms;
      for (int it = 0; it < 23; ++it) {
        CHK(hipEventRecord(e0, 0));
        if (form == 0) hipLaunchKernelGGL(k_global, dim3(blocks), dim3(256), 0, 0, d_rows, d_vw, d_eff, n, nc, G, o);
        else if (form == 1) hipLaunchKernelGGL(k_lds<1>, dim3(blocks), dim3(256), lds, 0, d_rows, d_vw, d_eff, n, nc, G, o);
        else if (form == 2) hipLaunchKernelGGL(k_lds<4>, dim3(blocks), dim3(256), lds, 0, d_rows, d_vw, d_eff, n, nc, G, o);
        else hipLaunchKernelGGL(k_lds<16>, dim3(blocks), dim3(256), lds, 0, d_rows, d_vw, d_eff, n, nc, G, o);
        CHK(hipGetLastError());
        CHK(hipEventRecord(e1, 0)); CHK(hipEventSynchronize(e1));
        float t; CHK(hipEventElapsedTime(&t, e0, e1));
        if (it >= 3) ms.push_back(t);
      }
      std::vector<uint64_t> got(G * nc);
      CHK(hipMemcpy(got.data(), o, 8 * got.size(), hipMemcpyDeviceToHost));
      if (form == 0) {                                     // the global form against the host, the LDS forms against it
        ref = got;
        for (size_t g = 0; g < G; g += 511)
          for (uint32_t q = 0; q < nc; ++q) {
            uint64_t w = 0;
            for (uint32_t i = 0; i < n; ++i) if ((rows[g * rb + (i >> 3)] >> (i & 7)) & 1) w += eff[(size_t)i * nc + q];
            if (w != got[g * nc + q]) { printf("MISMATCH against the host at group %zu\n", g); return 1; }
          }
      } else if (got != ref) { printf("MISMATCH between the forms\n"); return 1; }
      const float med = median_ms(ms);
      printf("%s  {\"cols\": %u, \"form\": \"%s\", \"groups_per_wave\": %d, \"lds_bytes\": %zu, \"median_us\": %.1f, \"min_us\": %.1f}", first ? "" : ",\n", nc,
             form ? "lds" : "global", gpw, form ? lds : (size_t)0, 1e3 * med, 1e3 * ms[0]);
      first = false;
    }
  }
  printf("\n]}}\n");
  return 0;
}
