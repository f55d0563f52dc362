// region_common.hpp — what the region growers share (region_grow.hip: normals; region_grow_rgb.hip: colours): the union-find over
// mutual edges, the label sweeps over one-way edges and the sizes by label.  DESIGN.md §4.17 has the labelling and its proof.
#pragma once

#include <algorithm>

#include "bvh_traverse.hpp"

namespace ope {
namespace {

constexpr int kRgBlock = 256;
constexpr uint32_t kNone = 0xffffffffu;
constexpr int kSweepBatch = 4;

__device__ __forceinline__ uint32_t ld_u32(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_u32(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the union-find of clusters.hip (path halving; the larger root hooked to the smaller by compare-and-swap)
__device__ __forceinline__ uint32_t uf_find(uint32_t *parent, uint32_t x) {
  for (;;) {
    const uint32_t p = ld_u32(parent + x);
    if (p == x) return x;
    const uint32_t g = ld_u32(parent + p);
    if (g != p) st_u32(parent + x, g);
    x = p == g ? p : g;
  }
}
__device__ void uf_union(uint32_t *parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a > b) { const uint32_t t = a; a = b; b = t; }
    uint32_t expect = b;
    if (__hip_atomic_compare_exchange_strong(parent + b, &expect, a, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  }
}

// 0. per point: its sorted position and its coordinates by ORIGINAL index (what the _cloud form gathers from)
__global__ __launch_bounds__(kRgBlock) void rg_pos_kernel(CloudView c, float4 *__restrict__ pts_by_o, uint32_t *__restrict__ pos_by_o) {
  const uint32_t p = blockIdx.x * kRgBlock + threadIdx.x;
  if (p >= c.n) return;
  const float4 q = c.xyzw[p];
  const uint32_t o = (uint32_t)__float_as_int(q.w);
  pts_by_o[o] = q;
  pos_by_o[o] = p;
}

// every point at its root (loads only, each thread writes its own entry: see cc_flatten_kernel)
__global__ __launch_bounds__(kRgBlock) void rg_flatten_kernel(uint32_t n_valid, uint32_t *__restrict__ parent) {
  const uint32_t x = blockIdx.x * kRgBlock + threadIdx.x;
  if (x >= n_valid) return;
  uint32_t r = ld_u32(parent + x);
  for (uint32_t q = ld_u32(parent + r); q != r; q = ld_u32(parent + r)) r = q;
  st_u32(parent + x, r);
}

// 4. one sweep: labels flow along the one-way edges between components, and every root jumps to its label's label.  Every value
// ever written to L[r] is the rank of a point that reaches r, so the order of the updates does not matter; a sweep that wrote
// nothing read a fixed point.  changed: this sweep's writes.
__global__ __launch_bounds__(kRgBlock) void rg_sweep_kernel(const uint32_t *__restrict__ ow, const uint32_t *__restrict__ rank_of_pos,
                                                            const uint32_t *__restrict__ parent, uint32_t n_valid, int k, uint32_t *__restrict__ L,
                                                            uint32_t *__restrict__ changed) {
  const uint32_t u = blockIdx.x * kRgBlock + threadIdx.x;   // a sorted position: ow's rows are by position, their entries ranks
  bool wrote = false;
  if (u < n_valid) {
    const uint32_t x = rank_of_pos[u], ru = parent[x];
    uint32_t lu = ld_u32(L + ru);
    if (ru == x) {
      const uint32_t t = ld_u32(L + parent[lu]);
      if (t < lu) { atomicMin(L + x, t); lu = t; wrote = true; }
    }
    for (int j = 0; j < k; ++j) {
      const uint32_t v = ow[(size_t)u * k + j];
      if (v == kNone) continue;
      const uint32_t rv = parent[v];
      if (rv != ru && lu < ld_u32(L + rv)) { atomicMin(L + rv, lu); wrote = true; }
    }
  }
  const unsigned long long m = __ballot(wrote);
  if (m && (threadIdx.x & 63u) == 0) atomicAdd(changed, (uint32_t)__popcll(m));
}

// 5a. label per point (a rank: its region's seed) and the region sizes, summed per wave and label before the atomic
__global__ __launch_bounds__(kRgBlock) void rg_size_kernel(const uint32_t *__restrict__ parent, const uint32_t *__restrict__ L, uint32_t n_valid,
                                                           uint32_t *__restrict__ lab, uint32_t *__restrict__ rsz) {
  const uint32_t x = blockIdx.x * kRgBlock + threadIdx.x;
  const bool on = x < n_valid;
  uint32_t l = kNone;
  if (on) { l = L[parent[x]]; lab[x] = l; }
  unsigned long long left = __ballot(on);
  while (left) {
    const int leader = __ffsll((long long)left) - 1;
    const uint32_t r = (uint32_t)__shfl((int)l, leader, 64);
    const unsigned long long grp = __ballot(on && l == r);
    if ((int)(threadIdx.x & 63u) == leader) atomicAdd(rsz + r, (uint32_t)__popcll(grp));
    left &= ~grp;
  }
}

int bits_for(unsigned long long v) {
  int b = 1;
  while (b < 64 && (v >> b) != 0ull) ++b;
  return b;
}
}  // namespace
}  // namespace ope
