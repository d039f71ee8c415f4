// k_inflate.hip -- compressed wire encodings to uncompressed ones with a verdict per element (inflate.h): one lane per element,
// the uncompressed bytes or the marker (0xFF in every byte) to `out`, 1 / 0 to `status` (may be null).  Own translation unit,
// field functions force-inlined (-DBN_FORCE_INLINE); the table of fp_pow_pm3_4 (14 field elements) lives in scratch.
#include "inflate.h"
#include "kernels.h"
using namespace bn;

BN_KERNEL k_g1_inflate(const uint8_t* in, size_t n, uint8_t* out, uint8_t* status) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool ok = g1_inflate(in + 32 * i, out + 64 * i);
  if (status) status[i] = ok ? 1 : 0;
}
BN_KERNEL k_g2_inflate(const uint8_t* in, size_t n, uint8_t* out, uint8_t* status) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool ok = g2_inflate(in + 64 * i, out + 128 * i);
  if (status) status[i] = ok ? 1 : 0;
}
