// morton.hpp — the key ope_cloud_upload sorts a cloud's points by (morton_order_device, sampling.hip), shared with the batched
// final pose (final_batch.hip), which puts its fine clouds in the same order on the device.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ope {

__device__ __forceinline__ uint32_t expand_bits10_dev(uint32_t v) {
  v = (v * 0x00010001u) & 0xFF0000FFu;
  v = (v * 0x00000101u) & 0x0F00F00Fu;
  v = (v * 0x00000011u) & 0xC30C30C3u;
  v = (v * 0x00000005u) & 0x49249249u;
  return v;
}

// 10 bits per axis over the cloud's bounding box (lo, iv = 1023.999 / extent, 0 for a flat axis); non-finite points 1 << 30, last
__device__ __forceinline__ uint32_t morton_code_dev(float x, float y, float z, float lox, float loy, float loz, float ivx, float ivy,
                                                   float ivz) {
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return 1u << 30;
  const uint32_t qx = min(1023u, (uint32_t)fmaxf(0.f, __fmul_rn(__fsub_rn(x, lox), ivx)));
  const uint32_t qy = min(1023u, (uint32_t)fmaxf(0.f, __fmul_rn(__fsub_rn(y, loy), ivy)));
  const uint32_t qz = min(1023u, (uint32_t)fmaxf(0.f, __fmul_rn(__fsub_rn(z, loz), ivz)));
  return expand_bits10_dev(qx) | (expand_bits10_dev(qy) << 1) | (expand_bits10_dev(qz) << 2);
}

}  // namespace ope
