// clusters.hip — Euclidean cluster extraction on the device (ope_euclidean_clusters, gfx950, wave64): the connected components
// of "d2 <= r2" over a cloud's finite points, as pcl::EuclideanClusterExtraction returns them (ObjectSegmentationPlane::getClusters,
// objectsegmentationplane.cpp:79-93).  DESIGN.md §4.10 has the algorithm and the proof of the cell margin.
//
//   1. every finite point gets the 64-bit id of its cell, edge h = kCellMargin * tol / sqrt(3) (cell coordinates in double); one
//      radix sort by cell id, the points entering in ORIGINAL order, so that a cell's points come by ascending index;
//   2. head flags, a scan and one pass give the occupied cells (m, device-side), their first point and a cell per point.  Two
//      points of one cell are always joined (the margin), so the union-find runs over cells;
//   3. one wave per cell looks up its 62 "forward" neighbours within +-2 cells (binary search in the sorted cell ids) and, when the
//      two cells do not share a root yet, compares their points 64 x 64 at a time until the first pair with d2 <= r2, then hooks
//      the larger root to the smaller (compare-and-swap).  Face neighbours run in a launch of their own first: most other pairs
//      then find one root and compare nothing.  A last launch flattens the forest;
//   4. per cell its size and smallest index (its first point) go to its root, summed per wave before one atomic per root and
//      wave; a sort by (size desc, smallest index asc) ranks the kept components; a scan gives the offsets; a stable sort by rank
//      of the points in ORIGINAL order gives every cluster's indices ascending.  One read-back.
// The _cloud form gathers every written cluster, takes its bounding box (one workgroup per cluster), sorts all clusters' points
// by (cluster, Morton code over its own box) in one radix sort and scatters them into the new clouds: what ope_cloud_select
// builds, without one call per cluster.
// The kernel launches and host synchronisations depend on n only, never on the number of clusters.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "coarse_stages.hpp"
#include "morton.hpp"
#include "stage_host.hpp"

namespace ope {
namespace {

constexpr int kCcBlock = 256;
constexpr int kCcWaves = kCcBlock / 64;
constexpr double kCellMargin = 0.999;   // h = kCellMargin * tol / sqrt(3): DESIGN §4.10 needs kCellMargin^2 < 1 - 1.3e-6
constexpr int kFaceOffsets = 3;
constexpr int kForwardOffsets = 62;
// the neighbours (dx, dy, dz) within +-2 cells whose cell id is larger (dz, then dy, then dx > 0): face neighbours first, then by distance
__constant__ signed char c_off[kForwardOffsets][3] = {
    {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {-1, 1, 0}, {1, 1, 0}, {0, -1, 1}, {-1, 0, 1}, {1, 0, 1}, {0, 1, 1}, {-1, -1, 1}, {1, -1, 1},
    {-1, 1, 1}, {1, 1, 1}, {2, 0, 0}, {0, 2, 0}, {0, 0, 2}, {-2, 1, 0}, {2, 1, 0}, {-1, 2, 0}, {1, 2, 0}, {0, -2, 1}, {-2, 0, 1},
    {2, 0, 1}, {0, 2, 1}, {0, -1, 2}, {-1, 0, 2}, {1, 0, 2}, {0, 1, 2}, {-1, -2, 1}, {1, -2, 1}, {-2, -1, 1}, {2, -1, 1}, {-2, 1, 1},
    {2, 1, 1}, {-1, 2, 1}, {1, 2, 1}, {-1, -1, 2}, {1, -1, 2}, {-1, 1, 2}, {1, 1, 2}, {-2, 2, 0}, {2, 2, 0}, {0, -2, 2}, {-2, 0, 2},
    {2, 0, 2}, {0, 2, 2}, {-2, -2, 1}, {2, -2, 1}, {-2, 2, 1}, {2, 2, 1}, {-1, -2, 2}, {1, -2, 2}, {-2, -1, 2}, {2, -1, 2}, {-2, 1, 2},
    {2, 1, 2}, {-1, 2, 2}, {1, 2, 2}, {-2, -2, 2}, {2, -2, 2}, {-2, 2, 2}, {2, 2, 2}};

struct CellGrid {
  double lo[3];
  double inv;                 // 1 / h
  unsigned long long dim[3];  // cells per axis (< 2^36); dim[0] * dim[1] * dim[2] < 2^62
};

__device__ __forceinline__ unsigned long long cell_axis(float v, double lo, double inv, unsigned long long dim) {
  const double t = floor(((double)v - lo) * inv);
  const unsigned long long i = t > 0.0 ? (unsigned long long)t : 0ull;
  return i < dim ? i : dim - 1ull;
}

// relaxed loads / stores of the union-find forest at device scope: they bypass the non-coherent per-CU cache, so that a wave sees
// the hooks other CUs made (a stale parent is still an ancestor: finds stay correct, the compare-and-swap decides)
__device__ __forceinline__ uint32_t ld_parent(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_parent(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint32_t uf_find(uint32_t *parent, uint32_t x) {
  for (;;) {   // path halving
    const uint32_t p = ld_parent(parent + x);
    if (p == x) return x;
    const uint32_t g = ld_parent(parent + p);
    if (g != p) st_parent(parent + x, g);
    x = p == g ? p : g;
  }
}

__device__ void uf_union(uint32_t *parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a > b) { const uint32_t t = a; a = b; b = t; }
    uint32_t expect = b;   // hook the larger root to the smaller
    if (__hip_atomic_compare_exchange_strong(parent + b, &expect, a, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  }
}

// FLANN's L2 order, no contraction: (dx*dx + dy*dy) + dz*dz in float
__device__ __forceinline__ float d2_flann(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// 1. cell id per point (ORIGINAL order): finite points their cell, the others `sentinel` (above every cell id); the point itself by
// original index, and its position in the cloud's sorted order
__global__ __launch_bounds__(kCcBlock) void cc_key_kernel(CloudView c, CellGrid g, unsigned long long sentinel, unsigned long long *__restrict__ keys,
                                                          uint32_t *__restrict__ vals, float4 *__restrict__ pts_by_o, uint32_t *__restrict__ pos_by_o) {
  const uint32_t p = blockIdx.x * kCcBlock + threadIdx.x;
  if (p >= c.n) return;
  const float4 q = c.xyzw[p];
  const uint32_t o = (uint32_t)__float_as_int(q.w);
  unsigned long long key = sentinel;
  if (p < c.n_valid) {
    const unsigned long long ix = cell_axis(q.x, g.lo[0], g.inv, g.dim[0]);
    const unsigned long long iy = cell_axis(q.y, g.lo[1], g.inv, g.dim[1]);
    const unsigned long long iz = cell_axis(q.z, g.lo[2], g.inv, g.dim[2]);
    key = (iz * g.dim[1] + iy) * g.dim[0] + ix;
  }
  keys[o] = key;
  vals[o] = o;
  pts_by_o[o] = q;
  pos_by_o[o] = p;
}

// 2a. head of a cell run (finite points only)
__global__ __launch_bounds__(kCcBlock) void cc_head_kernel(const unsigned long long *__restrict__ skey, uint32_t n_valid, uint32_t *__restrict__ head) {
  const uint32_t j = blockIdx.x * kCcBlock + threadIdx.x;
  if (j < n_valid) head[j] = (j == 0 || skey[j] != skey[j - 1]) ? 1u : 0u;
}

// 2b. (cid1 = inclusive scan of the heads) cells: first point, id, own parent; per point its cell and its coordinates in cell order;
// m = the occupied cells
__global__ __launch_bounds__(kCcBlock) void cc_cells_kernel(const unsigned long long *__restrict__ skey, const uint32_t *__restrict__ sval,
                                                            const uint32_t *__restrict__ cid1, const float4 *__restrict__ pts_by_o, uint32_t n,
                                                            uint32_t n_valid, uint32_t *__restrict__ cstart, unsigned long long *__restrict__ ckey,
                                                            uint32_t *__restrict__ parent, uint32_t *__restrict__ cellof, float4 *__restrict__ cpts,
                                                            uint32_t *__restrict__ d_m) {
  const uint32_t j = blockIdx.x * kCcBlock + threadIdx.x;
  if (j >= n) return;
  cpts[j] = pts_by_o[sval[j]];
  if (j >= n_valid) return;
  const uint32_t c = cid1[j] - 1u;
  cellof[j] = c;
  if (j == 0 || skey[j] != skey[j - 1]) {
    cstart[c] = j;
    ckey[c] = skey[j];
    parent[c] = c;
  }
  if (j == n_valid - 1) {
    cstart[c + 1] = n_valid;
    *d_m = c + 1;
  }
}

// 3. one wave per cell: its forward neighbours [o_begin, o_end) of c_off; a neighbour whose root differs gets its points compared
// with the cell's, 64 x 64, until the first joining pair.  pairs: cell pairs compared (one atomic per wave and launch)
__global__ __launch_bounds__(kCcBlock) void cc_link_kernel(const unsigned long long *__restrict__ ckey, const uint32_t *__restrict__ cstart,
                                                           const float4 *__restrict__ cpts, const uint32_t *__restrict__ d_m, CellGrid g, float r2,
                                                           int o_begin, int o_end, uint32_t *__restrict__ parent,
                                                           unsigned long long *__restrict__ pairs) {
  const uint32_t m = *d_m;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave0 = blockIdx.x * kCcWaves + (threadIdx.x >> 6), nwaves = gridDim.x * kCcWaves;
  uint32_t tested = 0;
  for (uint32_t c = wave0; c < m; c += nwaves) {
    const unsigned long long key = ckey[c];
    const long long ix = (long long)(key % g.dim[0]), t = (long long)(key / g.dim[0]);
    const long long iy = t % (long long)g.dim[1], iz = t / (long long)g.dim[1];
    // lane k: neighbour o_begin + k, found by binary search among the cells after c (forward neighbours have larger ids)
    int found = -1;
    const int k = o_begin + (int)lane;
    if (k < o_end) {
      const long long jx = ix + c_off[k][0], jy = iy + c_off[k][1], jz = iz + c_off[k][2];
      if (jx >= 0 && jy >= 0 && jz >= 0 && jx < (long long)g.dim[0] && jy < (long long)g.dim[1] && jz < (long long)g.dim[2]) {
        const unsigned long long nk = ((unsigned long long)jz * g.dim[1] + (unsigned long long)jy) * g.dim[0] + (unsigned long long)jx;
        uint32_t lo = c + 1u, hi = m;
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (ckey[mid] < nk) lo = mid + 1u; else hi = mid;
        }
        if (lo < m && ckey[lo] == nk) found = (int)lo;
      }
    }
    unsigned long long mask = __ballot(found >= 0);
    const uint32_t a0 = cstart[c], na = cstart[c + 1] - a0;
    while (mask) {
      const int src = __ffsll((long long)mask) - 1;
      mask &= mask - 1ull;
      const uint32_t d = (uint32_t)__builtin_amdgcn_readlane(found, src);
      // the root check runs in lane 0 and its answer is made wave-uniform: the ballots and the break below need every lane on one path
      int same = 0;
      if (lane == 0) same = uf_find(parent, c) == uf_find(parent, d) ? 1 : 0;
      if (__builtin_amdgcn_readfirstlane(same)) continue;
      ++tested;
      const uint32_t b0 = cstart[d], nb = cstart[d + 1] - b0;
      bool joined = false;
      for (uint32_t ia = 0; ia < na && !joined; ia += 64) {
        const bool va = ia + lane < na;
        const float4 a = va ? cpts[a0 + ia + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
        for (uint32_t ib = 0; ib < nb; ib += 64) {
          const uint32_t cnt = min(64u, nb - ib);
          const float4 b = ib + lane < nb ? cpts[b0 + ib + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
          bool hit = false;
          for (uint32_t s = 0; s < cnt; ++s) {
            const float bx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b.x), (int)s));
            const float by = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b.y), (int)s));
            const float bz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b.z), (int)s));
            hit |= d2_flann(a.x, a.y, a.z, bx, by, bz) <= r2;
          }
          if (__ballot(va && hit)) { joined = true; break; }
        }
      }
      if (joined && lane == 0) uf_union(parent, c, d);
    }
  }
  if (lane == 0 && tested) atomicAdd(pairs, (unsigned long long)tested);
}

// every cell points at its root.  Each thread walks up with loads only and writes its own cell alone: a path-halving find here
// could store a grandparent into a cell another thread has just pointed at its root, and that cell would be left off its root.
// (A cell read while another thread rewrites it holds either its old parent or its root: an ancestor either way.)
__global__ __launch_bounds__(kCcBlock) void cc_flatten_kernel(const uint32_t *__restrict__ d_m, uint32_t *__restrict__ parent) {
  const uint32_t m = *d_m;
  for (uint32_t c = blockIdx.x * kCcBlock + threadIdx.x; c < m; c += gridDim.x * kCcBlock) {
    uint32_t r = ld_parent(parent + c);
    for (uint32_t q = ld_parent(parent + r); q != r; q = ld_parent(parent + r)) r = q;
    st_parent(parent + c, r);
  }
}

// 4a. per cell: size and smallest index (its first point) to its root; the wave's cells sum per distinct root first
__global__ __launch_bounds__(kCcBlock) void cc_comp_kernel(const uint32_t *__restrict__ d_m, const uint32_t *__restrict__ parent,
                                                           const uint32_t *__restrict__ cstart, const float4 *__restrict__ cpts,
                                                           uint32_t *__restrict__ csize, uint32_t *__restrict__ cmin) {
  const uint32_t m = *d_m;
  const uint32_t c = blockIdx.x * kCcBlock + threadIdx.x;
  const bool on = c < m;
  uint32_t root = 0xffffffffu, sz = 0, mn = 0xffffffffu;
  if (on) {
    root = parent[c];
    sz = cstart[c + 1] - cstart[c];
    mn = (uint32_t)__float_as_int(cpts[cstart[c]].w);
  }
  unsigned long long left = __ballot(on);
  while (left) {
    const int leader = __ffsll((long long)left) - 1;
    const uint32_t r = (uint32_t)__shfl((int)root, leader, 64);
    const bool mine = on && root == r;
    const unsigned long long grp = __ballot(mine);
    uint32_t s = mine ? sz : 0u, lo = mine ? mn : 0xffffffffu;
    for (int off = 32; off >= 1; off >>= 1) {
      s += (uint32_t)__shfl_xor((int)s, off, 64);
      lo = min(lo, (uint32_t)__shfl_xor((int)lo, off, 64));
    }
    if ((int)(threadIdx.x & 63u) == leader) {
      atomicAdd(csize + r, s);
      atomicMin(cmin + r, lo);
    }
    left &= ~grp;
  }
}

// 4b. sort key per component slot i < n: roots (i < m) and the non-finite singletons (i >= n_valid: the point at sorted position i)
// that pass the size filter get ((n - size) << bn) | smallest index, every other slot `drop`
__global__ __launch_bounds__(kCcBlock) void cc_rank_key_kernel(const uint32_t *__restrict__ d_m, const uint32_t *__restrict__ parent,
                                                               const uint32_t *__restrict__ csize, const uint32_t *__restrict__ cmin,
                                                               const float4 *__restrict__ cpts, uint32_t n, uint32_t n_valid, int bn, uint32_t min_size,
                                                               uint32_t max_size, unsigned long long drop, unsigned long long *__restrict__ rkey,
                                                               uint32_t *__restrict__ rval) {
  const uint32_t m = *d_m;
  const uint32_t i = blockIdx.x * kCcBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t sz = 0, mn = 0;
  if (i < m && parent[i] == i) { sz = csize[i]; mn = cmin[i]; }
  else if (i >= n_valid) { sz = 1; mn = (uint32_t)__float_as_int(cpts[i].w); }
  const bool keep = sz >= 1 && sz >= min_size && sz <= max_size;
  rkey[i] = keep ? ((unsigned long long)(n - sz) << bn) | mn : drop;
  rval[i] = i;
}

// 4c. rank per kept component, sizes in rank order, K = the kept components
__global__ __launch_bounds__(kCcBlock) void cc_rank_kernel(const unsigned long long *__restrict__ rkey, const uint32_t *__restrict__ rval, uint32_t n, int bn,
                                                           unsigned long long drop, int32_t *__restrict__ rank_of, uint32_t *__restrict__ rsize,
                                                           uint32_t *__restrict__ d_K) {
  const uint32_t k = blockIdx.x * kCcBlock + threadIdx.x;
  if (k >= n) return;
  const unsigned long long key = rkey[k];
  if (key == drop) { rsize[k] = 0; return; }
  rank_of[rval[k]] = (int32_t)k;
  rsize[k] = n - (uint32_t)(key >> bn);
  if (k + 1 == n || rkey[k + 1] == drop) *d_K = k + 1;
}

// 4d. per point (ORIGINAL order): the written cluster holding it (rank < kcap) or -1; the key of the stable sort by rank
__global__ __launch_bounds__(kCcBlock) void cc_label_kernel(const float4 *__restrict__ cpts, const uint32_t *__restrict__ cellof,
                                                            const uint32_t *__restrict__ parent, const int32_t *__restrict__ rank_of, uint32_t n,
                                                            uint32_t n_valid, uint32_t kcap, int32_t *__restrict__ label, uint32_t *__restrict__ lkey,
                                                            uint32_t *__restrict__ lval) {
  const uint32_t j = blockIdx.x * kCcBlock + threadIdx.x;
  if (j >= n) return;
  const uint32_t o = (uint32_t)__float_as_int(cpts[j].w);
  const uint32_t comp = j < n_valid ? parent[cellof[j]] : j;
  const int32_t r = rank_of[comp];
  const bool written = r >= 0 && (uint32_t)r < kcap;
  label[o] = written ? r : -1;
  lkey[o] = written ? (uint32_t)r : kcap;
  lval[o] = o;
}

// ---- the _cloud form: one workgroup per written cluster k gathers its points (packed at roff[k], w = position in the cluster)
// and takes the bounding box of its finite points and their count: bb[k] = {lo xyz, hi xyz (ordered keys), finite count}
__global__ __launch_bounds__(kCcBlock) void cc_gather_box_kernel(const int32_t *__restrict__ idx, const uint32_t *__restrict__ roff,
                                                                 const float4 *__restrict__ pts_by_o, float4 *__restrict__ raw, uint32_t *__restrict__ clof,
                                                                 uint32_t *__restrict__ bb) {
  const uint32_t k = blockIdx.x, b = roff[k], e = roff[k + 1], t = threadIdx.x;
  uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u}, cnt = 0;
  for (uint32_t j = b + t; j < e; j += kCcBlock) {
    float4 q = pts_by_o[idx[j]];
    const float v[3] = {q.x, q.y, q.z};
    q.w = __int_as_float((int)(j - b));
    raw[j] = q;
    clof[j] = k;
    if (isfinite(q.x) && isfinite(q.y) && isfinite(q.z)) {
      ++cnt;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const uint32_t u = (uint32_t)__float_as_int(v[d]);
        const uint32_t key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
        lo[d] = min(lo[d], key);
        hi[d] = max(hi[d], key);
      }
    }
  }
  __shared__ uint32_t s_red[7][kCcWaves];
  const uint32_t w = t >> 6;
#pragma unroll
  for (int d = 0; d < 3; ++d)
    for (int off = 32; off >= 1; off >>= 1) {
      lo[d] = min(lo[d], (uint32_t)__shfl_xor((int)lo[d], off, 64));
      hi[d] = max(hi[d], (uint32_t)__shfl_xor((int)hi[d], off, 64));
    }
  for (int off = 32; off >= 1; off >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, off, 64);
  if ((t & 63u) == 0) {
    for (int d = 0; d < 3; ++d) { s_red[d][w] = lo[d]; s_red[3 + d][w] = hi[d]; }
    s_red[6][w] = cnt;
  }
  __syncthreads();
  if (t < 7) {
    uint32_t r = s_red[t][0];
    for (int q = 1; q < kCcWaves; ++q) r = t < 3 ? min(r, s_red[t][q]) : t < 6 ? max(r, s_red[t][q]) : r + s_red[t][q];
    bb[8 * k + t] = r;
  }
}

__device__ __forceinline__ float unkey_f(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  return __int_as_float((int)u);
}

// the box of cluster k as ope_cloud_select takes it: lo / hi of the finite points (0 0 0 if there are none), iv = 1023.999 / extent
__device__ __forceinline__ void cluster_box(const uint32_t *bb, uint32_t k, float lo[3], float iv[3]) {
  const bool any = bb[8 * k + 6] > 0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float l = any ? unkey_f(bb[8 * k + d]) : 0.f, h = any ? unkey_f(bb[8 * k + 3 + d]) : 0.f;
    lo[d] = l;
    iv[d] = h > l ? __fdiv_rn(1023.999f, __fsub_rn(h, l)) : 0.f;
  }
}

__global__ __launch_bounds__(kCcBlock) void cc_morton_key_kernel(const float4 *__restrict__ raw, const uint32_t *__restrict__ clof,
                                                                 const uint32_t *__restrict__ bb, uint32_t total, unsigned long long *__restrict__ keys,
                                                                 uint32_t *__restrict__ vals) {
  const uint32_t j = blockIdx.x * kCcBlock + threadIdx.x;
  if (j >= total) return;
  const uint32_t k = clof[j];
  float lo[3], iv[3];
  cluster_box(bb, k, lo, iv);
  const float4 q = raw[j];
  keys[j] = ((unsigned long long)k << 31) | morton_code_dev(q.x, q.y, q.z, lo[0], lo[1], lo[2], iv[0], iv[1], iv[2]);
  vals[j] = j;
}

struct ClusterOut { float4 *xyzw, *nrm; uint32_t *rgb; };

__global__ __launch_bounds__(kCcBlock) void cc_cloud_scatter_kernel(const unsigned long long *__restrict__ skey, const uint32_t *__restrict__ sval,
                                                                    const uint32_t *__restrict__ roff, const float4 *__restrict__ raw,
                                                                    const int32_t *__restrict__ idx, const uint32_t *__restrict__ pos_by_o,
                                                                    const float4 *__restrict__ nrm, const uint32_t *__restrict__ rgb,
                                                                    const ClusterOut *__restrict__ outs, uint32_t total) {
  const uint32_t q = blockIdx.x * kCcBlock + threadIdx.x;
  if (q >= total) return;
  const uint32_t k = (uint32_t)(skey[q] >> 31), j = sval[q], pos = q - roff[k];
  outs[k].xyzw[pos] = raw[j];
  if (nrm) outs[k].nrm[pos] = nrm[pos_by_o[idx[j]]];
  if (rgb) outs[k].rgb[pos] = rgb[pos_by_o[idx[j]]];   // the colour payload of the input, by its sorted position
}

int bits_for(unsigned long long v) {   // bits that hold every value <= v
  int b = 1;
  while (b < 64 && (v >> b) != 0ull) ++b;
  return b;
}

struct Result {
  uint32_t K = 0;                  // kept components
  std::vector<uint32_t> off;       // offsets of the written clusters (kw + 1)
  size_t kw = 0;                   // written clusters
};

int check_params(ope_ctx *ctx, const char *who, const ope_cloud *cloud, const ope_cluster_params *params, size_t *n_clusters,
                 ope_cluster_params &p) {
  if (!ctx) return OPE_EINVAL;
  ctx->cluster_stats = ope_cluster_stats{};
  if (!cloud || !n_clusters) return set_err(ctx, OPE_EINVAL, std::string(who) + "bad argument");
  ope_cluster_default_params(&p);
  if (params) p = *params;
  if (!(p.tolerance > 0.0) || !std::isfinite(p.tolerance) || !((float)p.tolerance > 0.f) || !std::isfinite((float)p.tolerance))
    return set_err(ctx, OPE_EINVAL, std::string(who) + "tolerance must be > 0 and finite");
  if (p.min_size < 1) return set_err(ctx, OPE_EINVAL, std::string(who) + "min_size must be >= 1");
  if (p.max_size < p.min_size) return set_err(ctx, OPE_EINVAL, std::string(who) + "max_size < min_size");
  if (cloud->n > (size_t)0x7fffffff) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than 2^31 - 1 points");
  return OPE_OK;
}

// the grid of a cloud: ERANGE when it would have 2^36 cells or more along an axis, or 2^62 or more in all
int make_grid(ope_ctx *ctx, const char *who, const ope_cloud *cloud, double tol_f, CellGrid &g) {
  const double h = kCellMargin * tol_f / std::sqrt(3.0);
  g.inv = 1.0 / h;
  long double cells = 1.0L;
  for (int d = 0; d < 3; ++d) {
    g.lo[d] = (double)cloud->bb_lo[d];
    const double t = std::floor(((double)cloud->bb_hi[d] - g.lo[d]) * g.inv);   // the device's expression at the box's far corner
    // (2^36 cells per axis keeps the rounding of the cell coordinate inside the margin: DESIGN §4.10)
    if (!(t >= 0.0) || t >= 68719476736.0) return set_err(ctx, OPE_ERANGE, std::string(who) + "the cloud spans 2^36 cells or more along an axis");
    g.dim[d] = (unsigned long long)t + 1ull;
    cells *= (long double)g.dim[d];
  }
  if (cells >= 4.611686018427387904e18L) return set_err(ctx, OPE_ERANGE, std::string(who) + "the cloud's grid would have 2^62 cells or more");
  return OPE_OK;
}

// Steps 1-4.  On success, the device buffers the _cloud form needs stay in tmp: *d_idx (the written clusters' points, packed),
// *d_roff (offsets), *d_pts_by_o, *d_pos_by_o.  want_idx / want_label: what comes back to the host.
int cluster_core(ope_ctx *ctx, CallTmp &tmp, const char *who, const ope_cloud *cloud, const ope_cluster_params &p, size_t max_clusters,
                 bool want_idx, int32_t *out_idx, int32_t *out_offsets, int32_t *out_label, Result &res, const int32_t **d_idx_out,
                 const uint32_t **d_roff_out, const float4 **d_pts_out, const uint32_t **d_pos_out) {
  ope_cluster_stats &St = ctx->cluster_stats;
  const uint32_t n = (uint32_t)cloud->n, n_valid = (uint32_t)cloud->n_valid;
  const float tol_f = (float)p.tolerance;
  const float r2 = (float)((double)tol_f * (double)tol_f);
  CellGrid g{};
  if (n_valid > 0) {
    const int rc = make_grid(ctx, who, cloud, (double)tol_f, g);
    if (rc != OPE_OK) return rc;
  } else {
    g.inv = 1.0; g.dim[0] = g.dim[1] = g.dim[2] = 1;
  }
  const unsigned long long n_cells = g.dim[0] * g.dim[1] * g.dim[2];
  const int cell_bits = bits_for(n_cells);           // cell ids < n_cells; the sentinel n_cells sorts last
  const int bn = bits_for(n);                         // n and every index fit
  const unsigned long long drop = (1ull << (2 * bn)) - 1ull;
  const size_t kcap = std::min<size_t>(max_clusters, n);
  const int lbits = bits_for(kcap);
  const hipStream_t st = ctx->stream;
  hipError_t e = hipSuccess;
  // buffers
  auto *keys = (unsigned long long *)tmp.get(8ull * n, e), *skey = (unsigned long long *)tmp.get(8ull * n, e);
  auto *vals = (uint32_t *)tmp.get(4ull * n, e), *sval = (uint32_t *)tmp.get(4ull * n, e);
  auto *pts_by_o = (float4 *)tmp.get(16ull * n, e);
  auto *pos_by_o = (uint32_t *)tmp.get(4ull * n, e);
  auto *head = (uint32_t *)tmp.get(4ull * n, e), *cid1 = (uint32_t *)tmp.get(4ull * n, e);
  auto *cstart = (uint32_t *)tmp.get(4ull * (n + 1), e);
  auto *ckey = (unsigned long long *)tmp.get(8ull * n, e);
  auto *parent = (uint32_t *)tmp.get(4ull * n, e), *cellof = (uint32_t *)tmp.get(4ull * n, e);
  auto *cpts = (float4 *)tmp.get(16ull * n, e);
  auto *csize = (uint32_t *)tmp.get(4ull * n, e), *cmin = (uint32_t *)tmp.get(4ull * n, e);
  auto *rank_of = (int32_t *)tmp.get(4ull * n, e);
  auto *rsize = (uint32_t *)tmp.get(4ull * (n + 1), e), *roff = (uint32_t *)tmp.get(4ull * (n + 1), e);
  auto *label = (int32_t *)tmp.get(4ull * n, e);
  auto *words = (unsigned long long *)tmp.get(32, e);   // [0] m | K (uint32 x 2), [1] pair tests
  auto *d_m = (uint32_t *)words, *d_K = (uint32_t *)words + 1;
  auto *pairs = words + 1;
  size_t tb = 0, t1 = 0;
  if (e == hipSuccess) e = rocprim::radix_sort_pairs(nullptr, t1, keys, skey, vals, sval, n, 0, 64, st);
  tb = std::max(tb, t1);
  if (e == hipSuccess) e = rocprim::inclusive_scan(nullptr, t1, head, cid1, n, rocprim::plus<uint32_t>(), st);
  tb = std::max(tb, t1);
  if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, t1, rsize, roff, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), st);
  tb = std::max(tb, t1);
  void *d_tmp = tmp.get(std::max<size_t>(tb, 16), e);
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  const CloudView cv = cloud->view();
  // 1. cell ids and the sort by cell
  if (e == hipSuccess) e = hipMemsetAsync(words, 0, 32, st);
  if (e == hipSuccess) e = hipMemsetAsync(csize, 0, 4ull * n, st);
  if (e == hipSuccess) e = hipMemsetAsync(cmin, 0xff, 4ull * n, st);
  if (e == hipSuccess) e = hipMemsetAsync(rank_of, 0xff, 4ull * n, st);
  if (e == hipSuccess) e = hipMemsetAsync(rsize + n, 0, 4, st);
  if (e == hipSuccess) e = hipMemsetAsync(cstart, 0, 4, st);
  St.launches += 6;
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  STAGE_LAUNCH(ctx, St.launches, cc_key_kernel, 40.0 * n, dim3(grid_of(n, kCcBlock)), dim3(kCcBlock), 0, st, cv, g, n_cells, keys, vals, pts_by_o, pos_by_o);
  STAGE_PRIM(ctx, St.launches, e, "cc_sort_cells", rocprim::radix_sort_pairs(d_tmp, (t1 = tb), keys, skey, vals, sval, n, 0, cell_bits, st));
  // 2. cells
  if (e == hipSuccess && n_valid > 0) {
    STAGE_LAUNCH(ctx, St.launches, cc_head_kernel, 20.0 * n_valid, dim3(grid_of(n_valid, kCcBlock)), dim3(kCcBlock), 0, st, skey, n_valid, head);
    STAGE_PRIM(ctx, St.launches, e, "cc_scan_cells", rocprim::inclusive_scan(d_tmp, (t1 = tb), head, cid1, n_valid, rocprim::plus<uint32_t>(), st));
  }
  STAGE_LAUNCH(ctx, St.launches, cc_cells_kernel, 60.0 * n, dim3(grid_of(n, kCcBlock)), dim3(kCcBlock), 0, st, skey, sval, cid1, pts_by_o, n, n_valid, cstart,
               ckey, parent, cellof, cpts, d_m);
  // 3. unions: face neighbours, the other forward neighbours, flatten
  const unsigned link_blocks = (unsigned)std::min<size_t>(std::max<size_t>(((size_t)n_valid + kCcWaves - 1) / kCcWaves, 1), (size_t)ctx->n_cu * 32);
  STAGE_LAUNCH(ctx, St.launches, cc_link_kernel, 0.0, dim3(link_blocks), dim3(kCcBlock), 0, st, ckey, cstart, cpts, d_m, g, r2, 0, kFaceOffsets, parent, pairs);
  STAGE_LAUNCH(ctx, St.launches, cc_link_kernel, 0.0, dim3(link_blocks), dim3(kCcBlock), 0, st, ckey, cstart, cpts, d_m, g, r2, kFaceOffsets, kForwardOffsets,
               parent, pairs);
  const unsigned flat_blocks = (unsigned)std::min<size_t>(grid_of(n_valid, kCcBlock), (size_t)ctx->n_cu * 16);
  STAGE_LAUNCH(ctx, St.launches, cc_flatten_kernel, 8.0 * n_valid, dim3(flat_blocks), dim3(kCcBlock), 0, st, d_m, parent);
  // 4. components, ranks, offsets, labels, indices by rank
  STAGE_LAUNCH(ctx, St.launches, cc_comp_kernel, 32.0 * n_valid, dim3(grid_of(n_valid, kCcBlock)), dim3(kCcBlock), 0, st, d_m, parent, cstart, cpts, csize,
               cmin);
  STAGE_LAUNCH(ctx, St.launches, cc_rank_key_kernel, 28.0 * n, dim3(grid_of(n, kCcBlock)), dim3(kCcBlock), 0, st, d_m, parent, csize, cmin, cpts, n, n_valid,
               bn, (uint32_t)p.min_size, (uint32_t)p.max_size, drop, keys, vals);
  STAGE_PRIM(ctx, St.launches, e, "cc_sort_ranks", rocprim::radix_sort_pairs(d_tmp, (t1 = tb), keys, skey, vals, sval, n, 0, 2 * bn, st));
  STAGE_LAUNCH(ctx, St.launches, cc_rank_kernel, 24.0 * n, dim3(grid_of(n, kCcBlock)), dim3(kCcBlock), 0, st, skey, sval, n, bn, drop, rank_of, rsize, d_K);
  STAGE_PRIM(ctx, St.launches, e, "cc_scan_offsets", rocprim::exclusive_scan(d_tmp, (t1 = tb), rsize, roff, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), st));
  auto *lkey = (uint32_t *)head, *lval = cid1, *lkey2 = (uint32_t *)csize, *idx = (uint32_t *)cmin;   // (free again by now)
  STAGE_LAUNCH(ctx, St.launches, cc_label_kernel, 36.0 * n, dim3(grid_of(n, kCcBlock)), dim3(kCcBlock), 0, st, cpts, cellof, parent, rank_of, n, n_valid,
               (uint32_t)kcap, label, lkey, lval);
  STAGE_PRIM(ctx, St.launches, e, "cc_sort_labels", rocprim::radix_sort_pairs(d_tmp, (t1 = tb), lkey, lkey2, lval, idx, n, 0, lbits, st));
  // the one read-back: m, K, pair tests, offsets, indices, labels
  unsigned long long hw[2] = {0, 0};
  std::vector<uint32_t> off(kcap + 1, 0);
  if (e == hipSuccess) e = hipMemcpyAsync(hw, words, 16, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(off.data(), roff, 4 * (kcap + 1), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && want_idx && n) e = hipMemcpyAsync(out_idx, idx, 4ull * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && out_label && n) e = hipMemcpyAsync(out_label, label, 4ull * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  ++St.host_syncs;
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  St.cells = (int64_t)(uint32_t)hw[0];
  St.pairs_tested = (int64_t)hw[1];
  res.K = (uint32_t)(hw[0] >> 32);
  res.kw = std::min<size_t>(res.K, kcap);
  off.resize(res.kw + 1);
  res.off = off;
  if (out_offsets)
    for (size_t k = 0; k <= res.kw; ++k) out_offsets[k] = (int32_t)off[k];
  *d_idx_out = (const int32_t *)idx;
  *d_roff_out = roff;
  *d_pts_out = pts_by_o;
  *d_pos_out = pos_by_o;
  return OPE_OK;
}

}  // namespace

// The tail of the _cloud forms (ope_euclidean_clusters_cloud, ope_region_grow_cloud): the kw written clusters (host offsets `off`,
// device offsets d_roff, packed ORIGINAL indices d_idx) as new device clouds, gathered, boxed, Morton-sorted and scattered in
// batched launches.  d_pts_by_o / d_pos_by_o: the input cloud's points and sorted positions by original index.
int clusters_build_clouds(ope_ctx *ctx, CallTmp &tmp, const char *who, const ope_cloud *cloud, size_t kw, const std::vector<uint32_t> &off,
                          const int32_t *d_idx, const uint32_t *d_roff, const float4 *d_pts, const uint32_t *d_pos, ope_cloud **out_clouds,
                          int64_t *launches, int64_t *host_syncs) {
  const uint32_t total = off[kw];
  // the new clouds, then every cluster's gather, box, Morton sort and scatter in batched launches
  std::vector<ope_cloud *> made(kw, nullptr);
  std::vector<ClusterOut> outs(kw);
  hipError_t e = hipSuccess;
  for (size_t k = 0; k < kw && e == hipSuccess; ++k) {
    ope_cloud *c = new ope_cloud();
    made[k] = c;
    c->ctx = ctx;
    c->n = off[k + 1] - off[k];
    c->host_valid = false;
    e = hipMalloc((void **)&c->d_xyzw, sizeof(float4) * std::max<size_t>(c->n, 1));
    if (e == hipSuccess && cloud->d_nrm) e = hipMalloc((void **)&c->d_nrm, sizeof(float4) * std::max<size_t>(c->n, 1));
    if (e == hipSuccess && cloud->d_rgb) e = hipMalloc((void **)&c->d_rgb, 4 * std::max<size_t>(c->n, 1));
    outs[k] = ClusterOut{c->d_xyzw, c->d_nrm, c->d_rgb};
  }
  auto *d_outs = (ClusterOut *)tmp.get(sizeof(ClusterOut) * kw, e);
  auto *raw = (float4 *)tmp.get(16ull * total, e);
  auto *clof = (uint32_t *)tmp.get(4ull * total, e);
  auto *bb = (uint32_t *)tmp.get(32ull * kw, e);
  auto *mkey = (unsigned long long *)tmp.get(8ull * total, e), *mkey2 = (unsigned long long *)tmp.get(8ull * total, e);
  auto *mval = (uint32_t *)tmp.get(4ull * total, e), *mval2 = (uint32_t *)tmp.get(4ull * total, e);
  const int mbits = 31 + bits_for(cloud->n);
  size_t tb = 0;
  if (e == hipSuccess) e = rocprim::radix_sort_pairs(nullptr, tb, mkey, mkey2, mval, mval2, total, 0, mbits, ctx->stream);
  void *d_tmp = tmp.get(std::max<size_t>(tb, 16), e);
  if (e == hipSuccess) { e = h2d_copy(ctx->stream, d_outs, outs.data(), sizeof(ClusterOut) * kw); ++*launches; }
  const hipStream_t st = ctx->stream;
  if (e == hipSuccess) {
    STAGE_LAUNCH(ctx, *launches, cc_gather_box_kernel, 24.0 * total, dim3((unsigned)kw), dim3(kCcBlock), 0, st, d_idx, d_roff, d_pts, raw, clof, bb);
    STAGE_LAUNCH(ctx, *launches, cc_morton_key_kernel, 32.0 * total, dim3(grid_of(total, kCcBlock)), dim3(kCcBlock), 0, st, raw, clof, bb, total, mkey, mval);
    STAGE_PRIM(ctx, *launches, e, "cc_sort_morton", rocprim::radix_sort_pairs(d_tmp, tb, mkey, mkey2, mval, mval2, total, 0, mbits, st));
  }
  if (e == hipSuccess)
    STAGE_LAUNCH(ctx, *launches, cc_cloud_scatter_kernel, 48.0 * total, dim3(grid_of(total, kCcBlock)), dim3(kCcBlock), 0, st, mkey2, mval2, d_roff, raw, d_idx,
                 d_pos, cloud->d_nrm, (const uint32_t *)cloud->d_rgb, d_outs, total);
  std::vector<uint32_t> h_bb(8 * kw);
  if (e == hipSuccess) e = hipMemcpyAsync(h_bb.data(), bb, 32ull * kw, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  ++*host_syncs;
  if (e != hipSuccess) {
    for (ope_cloud *c : made) ope_cloud_free(c);
    return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  }
  auto unkey = [](uint32_t k) { const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; float f; std::memcpy(&f, &u, 4); return f; };
  for (size_t k = 0; k < kw; ++k) {
    ope_cloud *c = made[k];
    c->n_valid = h_bb[8 * k + 6];
    for (int d = 0; d < 3; ++d) {
      c->bb_lo[d] = c->n_valid ? unkey(h_bb[8 * k + d]) : 0.f;
      c->bb_hi[d] = c->n_valid ? unkey(h_bb[8 * k + 3 + d]) : 0.f;
    }
    out_clouds[k] = c;
  }
  return OPE_OK;
}

}  // namespace ope

using namespace ope;

extern "C" {

void ope_cluster_default_params(ope_cluster_params *p) {
  if (!p) return;
  p->tolerance = 0.05;
  p->min_size = 300;
  p->max_size = 100000;
}

int ope_euclidean_clusters(ope_ctx *ctx, const ope_cloud *cloud, const ope_cluster_params *params, size_t max_clusters, size_t *n_clusters,
                           int32_t *out_idx, int32_t *out_offsets, int32_t *out_label) {
  static const char *who = "ope_euclidean_clusters: ";
  ope_cluster_params p;
  const int rc0 = check_params(ctx, who, cloud, params, n_clusters, p);
  if (rc0 != OPE_OK) return rc0;
  if (max_clusters > 0 && (!out_idx || !out_offsets)) return set_err(ctx, OPE_EINVAL, std::string(who) + "out_idx and out_offsets are required");
  *n_clusters = 0;
  if (out_offsets) out_offsets[0] = 0;
  if (cloud->n == 0) return OPE_OK;
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  TraceRange r(ctx, "euclidean_clusters");
  CallTmp tmp{ctx->stream, {}};
  Result res;
  const int32_t *d_idx; const uint32_t *d_roff, *d_pos; const float4 *d_pts;
  const int rc = cluster_core(ctx, tmp, who, cloud, p, max_clusters, max_clusters > 0, out_idx, out_offsets, out_label, res, &d_idx, &d_roff, &d_pts, &d_pos);
  if (rc != OPE_OK) return rc;
  *n_clusters = res.K;
  return OPE_OK;
}

int ope_euclidean_clusters_cloud(ope_ctx *ctx, const ope_cloud *cloud, const ope_cluster_params *params, size_t max_clusters, size_t *n_clusters,
                                 ope_cloud **out_clouds, int32_t *out_idx, int32_t *out_offsets) {
  static const char *who = "ope_euclidean_clusters_cloud: ";
  ope_cluster_params p;
  const int rc0 = check_params(ctx, who, cloud, params, n_clusters, p);
  if (rc0 != OPE_OK) return rc0;
  if (max_clusters > 0 && !out_clouds) return set_err(ctx, OPE_EINVAL, std::string(who) + "out_clouds is required");
  for (size_t k = 0; k < max_clusters; ++k) out_clouds[k] = nullptr;
  *n_clusters = 0;
  if (out_offsets) out_offsets[0] = 0;
  if (cloud->n == 0) return OPE_OK;
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  TraceRange r(ctx, "euclidean_clusters");
  CallTmp tmp{ctx->stream, {}};
  Result res;
  const int32_t *d_idx; const uint32_t *d_roff, *d_pos; const float4 *d_pts;
  int rc = cluster_core(ctx, tmp, who, cloud, p, max_clusters, out_idx != nullptr, out_idx, out_offsets, nullptr, res, &d_idx, &d_roff, &d_pts, &d_pos);
  if (rc != OPE_OK) return rc;
  if (res.kw > 0) {
    rc = clusters_build_clouds(ctx, tmp, who, cloud, res.kw, res.off, d_idx, d_roff, d_pts, d_pos, out_clouds, &ctx->cluster_stats.launches,
                               &ctx->cluster_stats.host_syncs);
    if (rc != OPE_OK) return rc;
  }
  *n_clusters = res.K;
  return OPE_OK;
}

int ope_cluster_last_stats(const ope_ctx *ctx, ope_cluster_stats *out) {
  if (!ctx || !out) return OPE_EINVAL;
  *out = ctx->cluster_stats;
  return OPE_OK;
}

}  // extern "C"
