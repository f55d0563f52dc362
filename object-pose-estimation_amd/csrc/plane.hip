// plane.hip — the table-top segmentation in front of the clusters (gfx950, wave64): pcl::SACSegmentation (SACMODEL_PLANE,
// SAC_RANSAC, optimised coefficients), pcl::ExtractPolygonalPrismData and the steps of
// ObjectSegmentationPlane::getSegmentedObjectsOnPlane between them (objectsegmentationplane.cpp:36-71, 122-235).  DESIGN.md §4.11
// has the float order of every step and why the replayed loop equals PCL's.
//
// ope_plane_segment:
//   1. one launch restores the cloud's ORIGINAL order (clouds are stored along the Morton curve, w = original index) and
//      fills shuffled_indices_ with 0..n-1;
//   2. one lane draws every sample RANSAC can reach (std::mt19937 in LDS, drawIndexSample's three swaps, isSampleGood with up to
//      1000 redraws) and computes each sample's plane: the draws do not depend on any inlier count;
//   3. one pass over the cloud scores all hypotheses: a lane loads its point once and tests it against every plane (the
//      coefficients in LDS), ballot / popcount per wave, one integer atomic per hypothesis and block;
//   4. the counts come back (first synchronisation) and the host replays RandomSampleConsensus::computeModel;
//   5. selectWithinDistance as flags by original index, a scan, the inliers' points packed in ascending index; one
//      workgroup runs computeMeanAndCovarianceMatrix's nine float sums IN INLIER ORDER (tiles staged in LDS, nine lanes each run
//      one sum down the tile: a sequential float sum cannot be split), eigen33 and the new d; selectWithinDistance again;
//   6. indices, count and coefficients come back (second synchronisation); the two clouds are cloud selections.
// ope_prism_extract: one lane takes the hull's plane, one launch tests every point, a scan and a scatter pack the survivors.
// ope_tabletop_segment chains them.  No launch count depends on the number of points or on the iterations the replay kept.
// ope_plane_peel (getSegmentedObjectsExceptPlane's loop, :296-319) runs steps 2-5 round after round on one packed
// point array: pl_peel_kernel, in step 5's last place, packs what a round leaves into the other half of a double buffer.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "coarse_stages.hpp"
#include "feature_math.hpp"
#include "stage_host.hpp"

namespace ope {
namespace {

constexpr int kPlBlock = 256;
constexpr int kMaxHyp = OPE_PLANE_MAX_ITERATIONS + 1;
constexpr int kMaxSampleChecks = 1000;   // SampleConsensusModel::max_sample_checks_
constexpr int kSelectLaunches = 4;       // what one cloud selection is counted as in the stats

// the plane distance of PCL's 4-vector dot product, in the one order the reference file fixes: ((a x + b y) + c z) + d, unfused
__device__ __forceinline__ float plane_dist(const float4 k, float x, float y, float z) {
  return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(k.x, x), __fmul_rn(k.y, y)), __fmul_rn(k.z, z)), k.w);
}
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
  return __fadd_rn(__fadd_rn(__fmul_rn(ax, bx), __fmul_rn(ay, by)), __fmul_rn(az, bz));
}

// the correctly rounded float square root (a double sqrt rounded to float)
__device__ __forceinline__ float sqrt_rn(float v) { return (float)__builtin_sqrt((double)v); }

// 1. original order, and (shuf != NULL) shuffled_indices_ = 0..n-1
__global__ __launch_bounds__(kPlBlock) void pl_orig_kernel(CloudView c, float4 *__restrict__ pts_o, int32_t *__restrict__ shuf) {
  const uint32_t p = blockIdx.x * kPlBlock + threadIdx.x;
  if (p >= c.n) return;
  const float4 q = c.xyzw[p];
  const uint32_t o = (uint32_t)__float_as_int(q.w);
  if (o < c.n) pts_o[o] = q;
  if (shuf) shuf[p] = (int32_t)p;
}

// std::mt19937, its 624 words in LDS
struct Mt {
  uint32_t *s;
  int i;
  __device__ void seed(uint32_t v) {
    s[0] = v;
    for (int k = 1; k < 624; ++k) s[k] = 1812433253u * (s[k - 1] ^ (s[k - 1] >> 30)) + (uint32_t)k;
    i = 624;
  }
  __device__ uint32_t next() {
    if (i >= 624) {
      for (int k = 0; k < 624; ++k) {
        const uint32_t y = (s[k] & 0x80000000u) | (s[(k + 1) % 624] & 0x7fffffffu);
        s[k] = s[(k + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
      }
      i = 0;
    }
    uint32_t y = s[i++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
  }
};

// SampleConsensusModelPlane::computeModelCoefficients: n = (p1 - p0) x (p2 - p0), normalised, d = -(n . p0)
__device__ float4 sample_plane(const float4 p0, const float4 p1, const float4 p2) {
  const float ax = __fsub_rn(p1.x, p0.x), ay = __fsub_rn(p1.y, p0.y), az = __fsub_rn(p1.z, p0.z);
  const float bx = __fsub_rn(p2.x, p0.x), by = __fsub_rn(p2.y, p0.y), bz = __fsub_rn(p2.z, p0.z);
  float nx = __fsub_rn(__fmul_rn(ay, bz), __fmul_rn(az, by));
  float ny = __fsub_rn(__fmul_rn(az, bx), __fmul_rn(ax, bz));
  float nz = __fsub_rn(__fmul_rn(ax, by), __fmul_rn(ay, bx));
  const float len = sqrt_rn(dot3(nx, ny, nz, nx, ny, nz));
  nx = __fdiv_rn(nx, len); ny = __fdiv_rn(ny, len); nz = __fdiv_rn(nz, len);
  return make_float4(nx, ny, nz, -dot3(nx, ny, nz, p0.x, p0.y, p0.z));
}

// 2. lane 0 draws H samples (or takes the n_inj injected ones) and computes their planes.  meta[0] = hypotheses made.
__global__ __launch_bounds__(64) void pl_draw_kernel(const float4 *__restrict__ pts_o, uint32_t n, int32_t *__restrict__ shuf, uint32_t seed,
                                                     uint32_t H, const int32_t *__restrict__ inj, uint32_t n_inj, float4 *__restrict__ hyp,
                                                     int32_t *__restrict__ samp, uint32_t *__restrict__ meta) {
  __shared__ uint32_t s_mt[624];
  if (threadIdx.x != 0) return;
  uint32_t made = 0;
  if (inj) {
    for (uint32_t h = 0; h < n_inj && h < H; ++h) {
      const int32_t a = inj[3 * h], b = inj[3 * h + 1], c = inj[3 * h + 2];
      samp[3 * h] = a; samp[3 * h + 1] = b; samp[3 * h + 2] = c;
      hyp[h] = sample_plane(pts_o[a], pts_o[b], pts_o[c]);
      ++made;
    }
  } else if (n >= 3) {
    Mt mt{s_mt, 624};
    mt.seed(seed);
    for (uint32_t h = 0; h < H; ++h) {
      bool good = false;
      int32_t a = 0, b = 0, c = 0;
      for (int check = 0; check < kMaxSampleChecks && !good; ++check) {
        for (uint32_t i = 0; i < 3; ++i) {   // drawIndexSample: swap(s[i], s[i + rnd() % (n - i)]), rnd() = engine() >> 1
          const uint32_t j = i + (uint32_t)((int32_t)(mt.next() >> 1) % (int32_t)(n - i));
          const int32_t t = shuf[i]; shuf[i] = shuf[j]; shuf[j] = t;
        }
        a = shuf[0]; b = shuf[1]; c = shuf[2];
        const float4 p0 = pts_o[a], p1 = pts_o[b], p2 = pts_o[c];
        // isSampleGood: r = (p1 - p0) / (p2 - p0) per component; good iff r0 != r1 || r2 != r1
        const float r0 = __fdiv_rn(__fsub_rn(p1.x, p0.x), __fsub_rn(p2.x, p0.x));
        const float r1 = __fdiv_rn(__fsub_rn(p1.y, p0.y), __fsub_rn(p2.y, p0.y));
        const float r2 = __fdiv_rn(__fsub_rn(p1.z, p0.z), __fsub_rn(p2.z, p0.z));
        good = (r0 != r1) || (r2 != r1);
        if (good) hyp[h] = sample_plane(p0, p1, p2);
      }
      if (!good) break;   // getSamples hands back an empty selection: the loop ends there
      samp[3 * h] = a; samp[3 * h + 1] = b; samp[3 * h + 2] = c;
      ++made;
    }
  }
  meta[0] = made;
}

// 3. countWithinDistance of every hypothesis in one pass: fabsf(dist) < threshold, the comparison in double.  The counts do not
// depend on the order of the points: pts is the cloud's stored array, or (the peel) a packed array of n points.
__global__ __launch_bounds__(kPlBlock) void pl_score_kernel(const float4 *__restrict__ pts, uint32_t n, const float4 *__restrict__ hyp,
                                                            const uint32_t *__restrict__ meta, double thr, uint32_t *__restrict__ cnt) {
  __shared__ float4 s_h[kMaxHyp];
  __shared__ uint32_t s_c[kMaxHyp];
  const uint32_t H = min(meta[0], (uint32_t)kMaxHyp), t = threadIdx.x;
  for (uint32_t i = t; i < H; i += kPlBlock) { s_h[i] = hyp[i]; s_c[i] = 0u; }
  __syncthreads();
  for (uint32_t base = blockIdx.x * kPlBlock; base < n; base += gridDim.x * kPlBlock) {
    const uint32_t p = base + t;
    const bool on = p < n;
    const float4 q = on ? pts[p] : make_float4(0.f, 0.f, 0.f, 0.f);
    for (uint32_t h = 0; h < H; ++h) {
      const float d = fabsf(plane_dist(s_h[h], q.x, q.y, q.z));
      const unsigned long long b = __ballot(on && (double)d < thr);
      if ((t & 63u) == 0 && b) atomicAdd(&s_c[h], (uint32_t)__popcll(b));
    }
  }
  __syncthreads();
  for (uint32_t i = t; i < H; i += kPlBlock)
    if (s_c[i]) atomicAdd(cnt + i, s_c[i]);
}

// 5a. selectWithinDistance as flags by ORIGINAL index (flags[n] = 0: the scan's last slot is the count)
__global__ __launch_bounds__(kPlBlock) void pl_flag_kernel(const float4 *__restrict__ pts_o, uint32_t n, const float4 *__restrict__ coeff, double thr,
                                                           uint32_t *__restrict__ flags) {
  const uint32_t o = blockIdx.x * kPlBlock + threadIdx.x;
  if (o > n) return;
  if (o == n) { flags[o] = 0u; return; }
  const float4 q = pts_o[o];
  flags[o] = (double)fabsf(plane_dist(*coeff, q.x, q.y, q.z)) < thr ? 1u : 0u;
}

// 5b. the flagged points packed in ascending index
__global__ __launch_bounds__(kPlBlock) void pl_pack_kernel(const float4 *__restrict__ pts_o, uint32_t n, const uint32_t *__restrict__ flags,
                                                           const uint32_t *__restrict__ rank, float4 *__restrict__ packed) {
  const uint32_t o = blockIdx.x * kPlBlock + threadIdx.x;
  if (o < n && flags[o]) packed[rank[o]] = pts_o[o];
}

// 5c. optimizeModelCoefficients: one workgroup.  Every thread stages the six products and three coordinates of one inlier, then
// lane a < 9 adds column a of the tile in inlier order.  out = the new coefficients (fewer than 4 inliers: the old ones).
__global__ __launch_bounds__(kPlBlock) void pl_refine_kernel(const float4 *__restrict__ packed, const uint32_t *__restrict__ d_m,
                                                             const float4 *__restrict__ coeff_in, float4 *__restrict__ out) {
  __shared__ float s_v[9][kPlBlock + 1];
  __shared__ float s_sum[9];
  const uint32_t m = *d_m, t = threadIdx.x;
  float acc = 0.f;
  for (uint32_t base = 0; base < m; base += kPlBlock) {
    const uint32_t cnt = min((uint32_t)kPlBlock, m - base);
    if (t < cnt) {
      const float4 q = packed[base + t];
      s_v[0][t] = __fmul_rn(q.x, q.x); s_v[1][t] = __fmul_rn(q.x, q.y); s_v[2][t] = __fmul_rn(q.x, q.z);
      s_v[3][t] = __fmul_rn(q.y, q.y); s_v[4][t] = __fmul_rn(q.y, q.z); s_v[5][t] = __fmul_rn(q.z, q.z);
      s_v[6][t] = q.x; s_v[7][t] = q.y; s_v[8][t] = q.z;
    }
    __syncthreads();
    if (t < 9) {
#pragma unroll 8
      for (uint32_t j = 0; j < cnt; ++j) acc = __fadd_rn(acc, s_v[t][j]);
    }
    __syncthreads();
  }
  if (t < 9) s_sum[t] = acc;
  __syncthreads();
  if (t != 0) return;
  if (m < 4) { *out = *coeff_in; return; }
  float accu[9];
  for (int a = 0; a < 9; ++a) accu[a] = s_sum[a];
  // (query and viewpoint both at the origin: normal_from_sums' flip never fires; PCL does not flip here)
  const float4 nv = normal_from_sums(accu, (int)m, make_float4(0.f, 0.f, 0.f, 0.f), 0.f, 0.f, 0.f);
  *out = make_float4(nv.x, nv.y, nv.z, -dot3(nv.x, nv.y, nv.z, accu[6], accu[7], accu[8]));   // accu[6..8]: the centroid by now
}

// 5d. the flagged indices ascending, and the others ascending
__global__ __launch_bounds__(kPlBlock) void pl_index_kernel(uint32_t n, const uint32_t *__restrict__ flags, const uint32_t *__restrict__ rank,
                                                            int32_t *__restrict__ idx, int32_t *__restrict__ rest) {
  const uint32_t o = blockIdx.x * kPlBlock + threadIdx.x;
  if (o >= n) return;
  if (flags[o]) idx[rank[o]] = (int32_t)o;
  else if (rest) rest[o - rank[o]] = (int32_t)o;
}

// ---- the peel.  Before its first round: orig = 0..n-1, every label -1
__global__ __launch_bounds__(kPlBlock) void pl_peel_init_kernel(uint32_t n, int32_t *__restrict__ orig, int32_t *__restrict__ label) {
  const uint32_t o = blockIdx.x * kPlBlock + threadIdx.x;
  if (o >= n) return;
  orig[o] = (int32_t)o;
  if (label) label[o] = -1;
}

// The peel's step, from a round's last flags / rank over its m points: the unflagged points and their original indices packed
// into the other half of the double buffer, ascending (what ExtractIndices' negative keeps, in order); label[original index] =
// round for the flagged ones; shuffled_indices_ = 0..m-1 again for the next round's draws; the next m left in *d_m.  One point
// per lane: 16 B loads and stores of the points, every other stream 4 B per lane and coalesced but the label's scatter.
__global__ __launch_bounds__(kPlBlock) void pl_peel_kernel(const float4 *__restrict__ pts, const int32_t *__restrict__ orig, uint32_t m,
                                                           const uint32_t *__restrict__ flags, const uint32_t *__restrict__ rank, int32_t round,
                                                           float4 *__restrict__ pts_next, int32_t *__restrict__ orig_next,
                                                           int32_t *__restrict__ label, int32_t *__restrict__ shuf, uint32_t *__restrict__ d_m) {
  const uint32_t o = blockIdx.x * kPlBlock + threadIdx.x;
  if (o == 0) *d_m = m - rank[m];
  if (o >= m) return;
  const uint32_t r = rank[o];
  const int32_t g = orig[o];
  if (flags[o]) {
    if (label) label[g] = round;
  } else {
    pts_next[o - r] = pts[o];
    orig_next[o - r] = g;
  }
  shuf[o] = (int32_t)o;
}

// ---- prism.  hp: {a b c d} of the hull's plane, {a' b' c' 0} its normal normalised once more (projectPoints), k1 k2 (int bits)
__global__ __launch_bounds__(64) void pl_hull_kernel(const float *__restrict__ hull, uint32_t m, float4 *__restrict__ hp) {
  if (threadIdx.x != 0) return;
  float accu[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (uint32_t v = 0; v < m; ++v) {
    const float x = hull[3 * v], y = hull[3 * v + 1], z = hull[3 * v + 2];
    accu[0] = __fadd_rn(accu[0], __fmul_rn(x, x)); accu[1] = __fadd_rn(accu[1], __fmul_rn(x, y)); accu[2] = __fadd_rn(accu[2], __fmul_rn(x, z));
    accu[3] = __fadd_rn(accu[3], __fmul_rn(y, y)); accu[4] = __fadd_rn(accu[4], __fmul_rn(y, z)); accu[5] = __fadd_rn(accu[5], __fmul_rn(z, z));
    accu[6] = __fadd_rn(accu[6], x); accu[7] = __fadd_rn(accu[7], y); accu[8] = __fadd_rn(accu[8], z);
  }
  const float4 nv = normal_from_sums(accu, (int)m, make_float4(0.f, 0.f, 0.f, 0.f), 0.f, 0.f, 0.f);
  float a = nv.x, b = nv.y, c = nv.z, d = -dot3(a, b, c, accu[6], accu[7], accu[8]);
  // flip towards the viewpoint (0 0 0): vp - hull[0]
  const float vx = __fsub_rn(0.f, hull[0]), vy = __fsub_rn(0.f, hull[1]), vz = __fsub_rn(0.f, hull[2]);
  if (dot3(vx, vy, vz, a, b, c) < 0.f) {
    a = -a; b = -b; c = -c;
    d = -dot3(a, b, c, hull[0], hull[1], hull[2]);
  }
  hp[0] = make_float4(a, b, c, d);
  const float len = sqrt_rn(dot3(a, b, c, a, b, c));
  hp[1] = make_float4(__fdiv_rn(a, len), __fdiv_rn(b, len), __fdiv_rn(c, len), 0.f);
  int k0 = (fabsf(a) > fabsf(b)) ? 0 : 1;
  const float ck0 = k0 == 0 ? a : b;
  k0 = (fabsf(ck0) > fabsf(c)) ? k0 : 2;
  hp[2] = make_float4(__int_as_float((k0 + 1) % 3), __int_as_float((k0 + 2) % 3), 0.f, 0.f);
}

__device__ __forceinline__ float pick3(float x, float y, float z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

__global__ __launch_bounds__(kPlBlock) void pl_prism_kernel(const float4 *__restrict__ pts_o, uint32_t n, const float4 *__restrict__ hp,
                                                            const float *__restrict__ hull, uint32_t m, double hmin, double hmax,
                                                            uint32_t *__restrict__ flags) {
  const uint32_t o = blockIdx.x * kPlBlock + threadIdx.x;
  if (o > n) return;
  if (o == n) { flags[o] = 0u; return; }
  const float4 q = pts_o[o];
  const float4 mc = hp[0], un = hp[1];
  const int k1 = __float_as_int(hp[2].x), k2 = __float_as_int(hp[2].y);
  const double dist = (double)plane_dist(mc, q.x, q.y, q.z);   // pointToPlaneDistanceSigned
  bool in = !(dist < hmin || dist > hmax);
  if (in) {
    // projectPoints: p - n' * (n' . p + d)
    const float dp = plane_dist(make_float4(un.x, un.y, un.z, mc.w), q.x, q.y, q.z);
    const float px = __fsub_rn(q.x, __fmul_rn(un.x, dp)), py = __fsub_rn(q.y, __fmul_rn(un.y, dp)), pz = __fsub_rn(q.z, __fmul_rn(un.z, dp));
    const double X = (double)pick3(px, py, pz, k1), Y = (double)pick3(px, py, pz, k2);
    // isXYPointIn2DXYPolygon: the crossing test, every edge once
    bool in_poly = false;
    double xold = (double)hull[3 * (m - 1) + k1], yold = (double)hull[3 * (m - 1) + k2];
    for (uint32_t v = 0; v < m; ++v) {
      const double xnew = (double)hull[3 * v + k1], ynew = (double)hull[3 * v + k2];
      double x1, y1, x2, y2;
      if (xnew > xold) { x1 = xold; x2 = xnew; y1 = yold; y2 = ynew; }
      else { x1 = xnew; x2 = xold; y1 = ynew; y2 = yold; }
      if ((xnew < X) == (X <= xold) && (Y - y1) * (x2 - x1) < (y2 - y1) * (X - x1)) in_poly = !in_poly;
      xold = xnew; yold = ynew;
    }
    in = in_poly;
  }
  flags[o] = in ? 1u : 0u;
}

// ---- table-top: the inliers projected into their plane (ProjectInliers), their extreme x and y as ordered keys
__global__ __launch_bounds__(kPlBlock) void pl_project_minmax_kernel(const float4 *__restrict__ pts_o, const int32_t *__restrict__ idx, uint32_t n_in,
                                                                     const float4 *__restrict__ coeff, uint32_t *__restrict__ mm) {
  const uint32_t j = blockIdx.x * kPlBlock + threadIdx.x;
  uint32_t lo[2] = {0xffffffffu, 0xffffffffu}, hi[2] = {0u, 0u};
  if (j < n_in) {
    const float4 q = pts_o[idx[j]], k = *coeff;
    const float len = sqrt_rn(dot3(k.x, k.y, k.z, k.x, k.y, k.z));
    const float ux = __fdiv_rn(k.x, len), uy = __fdiv_rn(k.y, len), uz = __fdiv_rn(k.z, len);
    const float dp = plane_dist(make_float4(ux, uy, uz, k.w), q.x, q.y, q.z);
    const float v[2] = {__fsub_rn(q.x, __fmul_rn(ux, dp)), __fsub_rn(q.y, __fmul_rn(uy, dp))};
#pragma unroll
    for (int d = 0; d < 2; ++d)
      if (v[d] == v[d]) {   // (getMinMax3D of finite points; a NaN never is an extreme)
        const uint32_t u = (uint32_t)__float_as_int(v[d]);
        lo[d] = hi[d] = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
      }
  }
#pragma unroll
  for (int d = 0; d < 2; ++d)
    for (int off = 32; off >= 1; off >>= 1) {
      lo[d] = min(lo[d], (uint32_t)__shfl_xor((int)lo[d], off, 64));
      hi[d] = max(hi[d], (uint32_t)__shfl_xor((int)hi[d], off, 64));
    }
  if ((threadIdx.x & 63u) == 0) {
    atomicMin(mm + 0, lo[0]); atomicMin(mm + 1, lo[1]);
    atomicMax(mm + 2, hi[0]); atomicMax(mm + 3, hi[1]);
  }
}

// out[j] = outer[inner[j]]
__global__ __launch_bounds__(kPlBlock) void pl_compose_kernel(const int32_t *__restrict__ outer, const int32_t *__restrict__ inner, uint32_t n,
                                                              int32_t *__restrict__ out) {
  const uint32_t j = blockIdx.x * kPlBlock + threadIdx.x;
  if (j < n) out[j] = outer[inner[j]];
}

int check_plane_params(ope_ctx *ctx, const char *who, const ope_plane_params *params, ope_plane_params &p) {
  ope_plane_default_params(&p);
  if (params) p = *params;
  if (!(p.distance_threshold >= 0.0) || !std::isfinite(p.distance_threshold))
    return set_err(ctx, OPE_EINVAL, std::string(who) + "distance_threshold must be >= 0 and finite");
  if (!(p.probability > 0.0 && p.probability < 1.0)) return set_err(ctx, OPE_EINVAL, std::string(who) + "probability must be inside (0, 1)");
  if (p.max_iterations < 0 || p.max_iterations > OPE_PLANE_MAX_ITERATIONS)
    return set_err(ctx, OPE_EINVAL, std::string(who) + "max_iterations must be 0 .. OPE_PLANE_MAX_ITERATIONS");
  return OPE_OK;
}

struct Fit {
  bool found = false;
  float coeff[4] = {0, 0, 0, 0};
  uint32_t n_in = 0;
  int32_t *d_idx = nullptr, *d_rest = nullptr;   // inliers / the others, ascending (in tmp)
  float4 *d_pts_o = nullptr;                     // the cloud in original order (in tmp)
  float4 *d_coeff = nullptr;                     // the returned coefficients on the device
};

// the exclusive scan of n + 1 flags: rank[o] = flagged points before o, rank[n] = their count
hipError_t scan_flags(ope_ctx *ctx, void *d_tmp, size_t tb, const uint32_t *flags, uint32_t *rank, size_t n) {
  KernelTimer kt(ctx, "pl_scan", 8.0 * n);
  ++ctx->plane_stats.launches;
  return rocprim::exclusive_scan(d_tmp, tb, flags, rank, 0u, n + 1, rocprim::plus<uint32_t>(), ctx->stream);
}

// the temporaries of one fit of at most n points and H hypotheses; the peel keeps one set for all its rounds
struct FitBufs {
  float4 *pts_o = nullptr, *packed = nullptr, *d_coeff = nullptr;
  int32_t *shuf = nullptr, *idx = nullptr, *rest = nullptr, *d_inj = nullptr;
  unsigned char *d_back = nullptr;   // one block read back at the first synchronisation: hyp (H float4) | samp (3H) | cnt (H) | meta (4 words)
  size_t back_bytes = 0, tb = 0;
  uint32_t *flags = nullptr, *rank = nullptr;
  void *d_tmp = nullptr;
};

hipError_t fit_alloc(CallTmp &tmp, hipStream_t st, uint32_t n, uint32_t H, bool injected, size_t n_samples, bool index, FitBufs &B) {
  hipError_t e = hipSuccess;
  const size_t n1 = std::max<size_t>(n, 1);
  B.pts_o = (float4 *)tmp.get(16 * n1, e);
  B.shuf = (int32_t *)tmp.get(4 * n1, e);
  B.back_bytes = 16ull * H + 12ull * H + 4ull * H + 16;
  B.d_back = (unsigned char *)tmp.get(B.back_bytes, e);
  B.flags = (uint32_t *)tmp.get(4 * (n1 + 1), e);
  B.rank = (uint32_t *)tmp.get(4 * (n1 + 1), e);
  B.packed = (float4 *)tmp.get(16 * n1, e);
  if (index) {
    B.idx = (int32_t *)tmp.get(4 * n1, e);
    B.rest = (int32_t *)tmp.get(4 * n1, e);
  }
  B.d_coeff = (float4 *)tmp.get(16, e);
  if (injected) B.d_inj = (int32_t *)tmp.get(12 * std::max<size_t>(n_samples, 1), e);
  if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, B.tb, B.flags, B.rank, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), st);
  B.tb = std::max<size_t>(B.tb, 16);
  B.d_tmp = tmp.get(B.tb, e);
  return e;
}

// what a round of the peel runs in place of pl_index_kernel (pl_peel_kernel's arguments)
struct PeelStep {
  float4 *pts_next;
  const int32_t *orig;
  int32_t *orig_next, *label;
  int32_t round;
  uint32_t *d_m;
  uint32_t m_next;   // out: *d_m, read back at the second synchronisation
};

// steps 1-6 without the clouds, on n points.  cloud: the points' source (step 1 restores its original order into B.pts_o); NULL
// (the peel after its first round): B.pts_o holds them already and B.shuf is 0..n-1.  samples: host triples or null.  peel: the
// step that takes pl_index_kernel's place.  Adds to ctx->plane_stats' launches and syncs; sets the rest.
int fit_run(ope_ctx *ctx, const char *who, const FitBufs &B, const ope_cloud *cloud, uint32_t n, const ope_plane_params &p, const int32_t *samples,
            size_t n_samples, int32_t *out_idx, PeelStep *peel, Fit &fit) {
  const uint32_t H = (uint32_t)p.max_iterations + 1u;
  const hipStream_t st = ctx->stream;
  ope_plane_stats &S = ctx->plane_stats;
  S.iterations = S.hypotheses = 0;
  S.best = -1;
  S.found = 0;
  ctx->plane_samples.clear(); ctx->plane_counts.clear(); ctx->plane_coeffs.clear();
  hipError_t e = hipSuccess;
  float4 *pts_o = B.pts_o, *packed = B.packed, *d_coeff = B.d_coeff;
  int32_t *shuf = B.shuf, *idx = B.idx, *rest = B.rest, *d_inj = B.d_inj;
  unsigned char *d_back = B.d_back;
  const size_t back_bytes = B.back_bytes;
  uint32_t *flags = B.flags, *rank = B.rank;
  void *d_tmp = B.d_tmp;
  size_t tb = B.tb;
  if (peel) {   // fewer points than the buffers were sized for: a query (nothing is launched) that the scan still fits
    e = rocprim::exclusive_scan(nullptr, tb, flags, rank, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), st);
    if (e != hipSuccess || tb > B.tb)
      return set_err(ctx, OPE_EHIP, std::string(who) + (e != hipSuccess ? hipGetErrorString(e) : "the scan's temporary storage grew with fewer points"));
    tb = B.tb;
  }
  auto *hyp = (float4 *)d_back;
  auto *samp = (int32_t *)(d_back + 16ull * H);
  auto *cnt = (uint32_t *)(d_back + 28ull * H);
  auto *meta = (uint32_t *)(d_back + 32ull * H);
  fit.d_pts_o = pts_o;
  fit.d_idx = idx;
  fit.d_rest = rest;
  fit.d_coeff = d_coeff;
  if (samples) {
    for (size_t j = 0; j < 3 * n_samples; ++j)
      if (samples[j] < 0 || (uint32_t)samples[j] >= n) return set_err(ctx, OPE_EINVAL, std::string(who) + "sample index out of range");
    if (n_samples) e = h2d_copy(st, d_inj, samples, 12 * n_samples);
  }
  if (e == hipSuccess) e = hipMemsetAsync(d_back, 0, back_bytes, st);
  ++S.launches;
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  if (cloud) STAGE_LAUNCH(ctx, S.launches, pl_orig_kernel, 36.0 * n, dim3(grid_of(n, kPlBlock)), dim3(kPlBlock), 0, st, cloud->view(), pts_o, shuf);
  STAGE_LAUNCH(ctx, S.launches, pl_draw_kernel, 0.0, dim3(1), dim3(64), 0, st, pts_o, n, shuf, (uint32_t)(p.seed & 0xffffffffull), H, d_inj,
               (uint32_t)n_samples, hyp, samp, meta);
  const unsigned score_blocks = (unsigned)std::min<size_t>(grid_of(n, kPlBlock), (size_t)ctx->n_cu * 8);
  STAGE_LAUNCH(ctx, S.launches, pl_score_kernel, 16.0 * n, dim3(score_blocks), dim3(kPlBlock), 0, st,
               cloud ? (const float4 *)cloud->d_xyzw : (const float4 *)pts_o, n, hyp, meta, p.distance_threshold, cnt);
  // ---- the first synchronisation: hypotheses and counts
  std::vector<unsigned char> back(back_bytes);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(back.data(), d_back, back_bytes, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  ++S.host_syncs;
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  uint32_t made = 0;
  std::memcpy(&made, back.data() + 32ull * H, 4);
  made = std::min(made, H);
  ctx->plane_coeffs.resize(4 * (size_t)made);
  ctx->plane_samples.resize(3 * (size_t)made);
  ctx->plane_counts.resize(made);
  std::memcpy(ctx->plane_coeffs.data(), back.data(), 16ull * made);
  std::memcpy(ctx->plane_samples.data(), back.data() + 16ull * H, 12ull * made);
  std::memcpy(ctx->plane_counts.data(), back.data() + 28ull * H, 4ull * made);
  S.hypotheses = made;
  // ---- RandomSampleConsensus::computeModel, replayed: the draws did not depend on the counts, so hypothesis `it` is the one
  // iteration `it` would have drawn
  int best = -1;
  long long best_cnt = -(long long)INT_MAX;
  double k = 1.0;
  int it = 0;
  const double log_probability = std::log(1.0 - p.probability);
  while ((double)it < k) {
    if ((uint32_t)it >= made) break;   // an empty selection
    const long long c = ctx->plane_counts[it];
    if (c > best_cnt) {
      best_cnt = c;
      best = it;
      const double w = (double)best_cnt / (double)n;
      double p_no_outliers = 1.0 - std::pow(w, 3.0);
      p_no_outliers = std::max(DBL_EPSILON, p_no_outliers);
      p_no_outliers = std::min(1.0 - DBL_EPSILON, p_no_outliers);
      k = log_probability / std::log(p_no_outliers);
    }
    ++it;
    if (it > p.max_iterations) break;
  }
  S.iterations = it;
  S.best = best;
  if (best < 0) return OPE_OK;   // no model
  S.found = 1;
  fit.found = true;
  // ---- inliers, refinement, inliers again
  const float4 *c_best = hyp + best;
  const float4 *c_final = c_best;
  if (p.optimize_coefficients) {
    STAGE_LAUNCH(ctx, S.launches, pl_flag_kernel, 20.0 * n, dim3(grid_of((size_t)n + 1, kPlBlock)), dim3(kPlBlock), 0, st, pts_o, n, c_best,
                 p.distance_threshold, flags);
    e = scan_flags(ctx, d_tmp, tb, flags, rank, n);
    if (e == hipSuccess) {
      STAGE_LAUNCH(ctx, S.launches, pl_pack_kernel, 40.0 * n, dim3(grid_of(n, kPlBlock)), dim3(kPlBlock), 0, st, pts_o, n, flags, rank, packed);
      STAGE_LAUNCH(ctx, S.launches, pl_refine_kernel, 16.0 * n, dim3(1), dim3(kPlBlock), 0, st, packed, rank + n, c_best, d_coeff);
    }
    c_final = d_coeff;
  } else if (e == hipSuccess) {
    e = hipMemcpyAsync(d_coeff, c_best, 16, hipMemcpyDeviceToDevice, st);
    ++S.launches;
  }
  if (e == hipSuccess) {
    STAGE_LAUNCH(ctx, S.launches, pl_flag_kernel, 20.0 * n, dim3(grid_of((size_t)n + 1, kPlBlock)), dim3(kPlBlock), 0, st, pts_o, n, c_final,
                 p.distance_threshold, flags);
    e = scan_flags(ctx, d_tmp, tb, flags, rank, n);
  }
  if (e == hipSuccess && !peel)
    STAGE_LAUNCH(ctx, S.launches, pl_index_kernel, 16.0 * n, dim3(grid_of(n, kPlBlock)), dim3(kPlBlock), 0, st, n, flags, rank, idx, rest);
  if (e == hipSuccess && peel)
    STAGE_LAUNCH(ctx, S.launches, pl_peel_kernel, 52.0 * n, dim3(grid_of(n, kPlBlock)), dim3(kPlBlock), 0, st, pts_o, peel->orig, n, flags, rank, peel->round,
                 peel->pts_next, peel->orig_next, peel->label, shuf, peel->d_m);
  // ---- the second synchronisation: coefficients, count (and the indices, whose number the host does not know yet)
  uint32_t n_in = 0;
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(fit.coeff, d_coeff, 16, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(&n_in, rank + n, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && peel) e = hipMemcpyAsync(&peel->m_next, peel->d_m, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && out_idx) e = hipMemcpyAsync(out_idx, idx, 4ull * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  ++S.host_syncs;
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  fit.n_in = n_in;
  return OPE_OK;
}

int plane_fit(ope_ctx *ctx, CallTmp &tmp, const char *who, const ope_cloud *cloud, const ope_plane_params &p, const int32_t *samples,
              size_t n_samples, int32_t *out_idx, Fit &fit) {
  FitBufs B;
  const hipError_t e = fit_alloc(tmp, ctx->stream, (uint32_t)cloud->n, (uint32_t)p.max_iterations + 1u, samples != nullptr, n_samples, true, B);
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  return fit_run(ctx, who, B, cloud, (uint32_t)cloud->n, p, samples, n_samples, out_idx, nullptr, fit);
}

// a selection, counted
int select_counted(ope_ctx *ctx, const ope_cloud *cloud, const int32_t *d_idx, size_t n_sel, ope_cloud **out) {
  ctx->plane_stats.launches += kSelectLaunches;
  ctx->plane_stats.host_syncs += cloud->d_nrm ? 2 : 1;
  return select_cloud_device(ctx, cloud, d_idx, n_sel, out);
}

// the prism's survivors of `cloud` (pts_o: its original order): *d_idx_out (in tmp) ascending, *count on the host (one synchronisation)
int prism_run(ope_ctx *ctx, CallTmp &tmp, const char *who, const ope_cloud *cloud, const float4 *pts_o, const float *hull, size_t m, double hmin,
              double hmax, int32_t **d_idx_out, uint32_t *count, int32_t *out_idx, float hull_coeff[4]) {
  const uint32_t n = (uint32_t)cloud->n;
  const hipStream_t st = ctx->stream;
  hipError_t e = hipSuccess;
  const size_t n1 = std::max<size_t>(n, 1);
  auto *d_hull = (float *)tmp.get(12 * m, e);
  auto *hp = (float4 *)tmp.get(48, e);
  auto *flags = (uint32_t *)tmp.get(4 * (n1 + 1), e), *rank = (uint32_t *)tmp.get(4 * (n1 + 1), e);
  auto *idx = (int32_t *)tmp.get(4 * n1, e);
  size_t tb = 0;
  if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, tb, flags, rank, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), st);
  void *d_tmp = tmp.get(std::max<size_t>(tb, 16), e);
  if (e == hipSuccess) { e = h2d_copy(st, d_hull, hull, 12 * m); ++ctx->plane_stats.launches; }
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  STAGE_LAUNCH(ctx, ctx->plane_stats.launches, pl_hull_kernel, 0.0, dim3(1), dim3(64), 0, st, d_hull, (uint32_t)m, hp);
  STAGE_LAUNCH(ctx, ctx->plane_stats.launches, pl_prism_kernel, 20.0 * n, dim3(grid_of((size_t)n + 1, kPlBlock)), dim3(kPlBlock), 0, st, pts_o, n, hp, d_hull,
               (uint32_t)m, hmin, hmax, flags);
  e = scan_flags(ctx, d_tmp, tb, flags, rank, n);
  if (e == hipSuccess)
    STAGE_LAUNCH(ctx, ctx->plane_stats.launches, pl_index_kernel, 12.0 * n, dim3(grid_of(n, kPlBlock)), dim3(kPlBlock), 0, st, n, flags, rank, idx,
                 (int32_t *)nullptr);
  float hc[4] = {0, 0, 0, 0};
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(count, rank + n, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(hc, hp, 16, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && out_idx && n) e = hipMemcpyAsync(out_idx, idx, 4ull * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  ++ctx->plane_stats.host_syncs;
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  if (hull_coeff) std::memcpy(hull_coeff, hc, 16);
  *d_idx_out = idx;
  return OPE_OK;
}

float unkey_host(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

}  // namespace
}  // namespace ope

using namespace ope;

extern "C" {

void ope_plane_default_params(ope_plane_params *p) {
  if (!p) return;
  p->distance_threshold = 0.01;
  p->probability = 0.99;
  p->max_iterations = 50;
  p->optimize_coefficients = 1;
  p->seed = 12345;
}

int ope_plane_segment(ope_ctx *ctx, const ope_cloud *cloud, const ope_plane_params *params, const int32_t *samples, size_t n_samples,
                      float coeff[4], int32_t *out_idx, size_t *n_inliers, ope_cloud **plane, ope_cloud **not_plane) {
  static const char *who = "ope_plane_segment: ";
  if (!ctx) return OPE_EINVAL;
  ctx->plane_stats = ope_plane_stats{};
  ctx->plane_stats.best = -1;
  if (plane) *plane = nullptr;
  if (not_plane) *not_plane = nullptr;
  if (!cloud || !coeff || !n_inliers || (n_samples && !samples)) return set_err(ctx, OPE_EINVAL, std::string(who) + "bad argument");
  ope_plane_params p;
  { const int rc = check_plane_params(ctx, who, params, p); if (rc != OPE_OK) return rc; }
  if (samples && n_samples > (size_t)p.max_iterations + 1) return set_err(ctx, OPE_EINVAL, std::string(who) + "more samples than max_iterations + 1");
  if (cloud->n > (size_t)0x7fffffff) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than 2^31 - 1 points");
  *n_inliers = 0;
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  TraceRange r(ctx, "plane_segment");
  CallTmp tmp{ctx->stream, {}};
  Fit fit;
  int rc = plane_fit(ctx, tmp, who, cloud, p, samples, n_samples, out_idx, fit);
  if (rc != OPE_OK) return rc;
  if (fit.found) {
    std::memcpy(coeff, fit.coeff, 16);
    *n_inliers = fit.n_in;
  }
  if (plane) rc = select_counted(ctx, cloud, fit.found ? fit.d_idx : nullptr, fit.found ? fit.n_in : 0, plane);
  if (rc == OPE_OK && not_plane) {
    if (fit.found) rc = select_counted(ctx, cloud, fit.d_rest, cloud->n - fit.n_in, not_plane);
    else {   // no model: ExtractIndices (negative) of an empty list is every point
      std::vector<int32_t> all(cloud->n);
      for (size_t i = 0; i < all.size(); ++i) all[i] = (int32_t)i;
      ctx->plane_stats.launches += kSelectLaunches;
      ctx->plane_stats.host_syncs += cloud->d_nrm ? 2 : 1;
      rc = ope_cloud_select(ctx, cloud, all.data(), all.size(), not_plane);
    }
    if (rc != OPE_OK && plane && *plane) { ope_cloud_free(*plane); *plane = nullptr; }
  }
  return rc;
}

void ope_peel_default_params(ope_peel_params *p) {
  if (!p) return;
  p->keep_fraction = 0.3;
  p->max_planes = 0;
}

int ope_plane_peel(ope_ctx *ctx, const ope_cloud *cloud, const ope_plane_params *plane, const ope_peel_params *peel, size_t cap_planes,
                   float *coeffs, int32_t *counts, int64_t *iterations, int32_t *label, int32_t *rest_idx, ope_cloud **rest,
                   ope_peel_result *out) {
  static const char *who = "ope_plane_peel: ";
  if (!ctx) return OPE_EINVAL;
  ctx->plane_stats = ope_plane_stats{};
  ctx->plane_stats.best = -1;
  ctx->plane_samples.clear(); ctx->plane_counts.clear(); ctx->plane_coeffs.clear();
  if (rest) *rest = nullptr;
  if (out) std::memset(out, 0, sizeof *out);
  if (!cloud || !out) return set_err(ctx, OPE_EINVAL, std::string(who) + "bad argument");
  ope_plane_params p;
  { const int rc = check_plane_params(ctx, who, plane, p); if (rc != OPE_OK) return rc; }
  ope_peel_params q;
  ope_peel_default_params(&q);
  if (peel) q = *peel;
  if (!std::isfinite(q.keep_fraction) || q.keep_fraction < 0.0) return set_err(ctx, OPE_EINVAL, std::string(who) + "keep_fraction must be >= 0 and finite");
  if (q.max_planes < 0) return set_err(ctx, OPE_EINVAL, std::string(who) + "max_planes must be >= 0");
  if (cloud->n > (size_t)0x7fffffff) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than 2^31 - 1 points");
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  TraceRange r(ctx, "plane_peel");
  CallTmp tmp{ctx->stream, {}};
  const hipStream_t st = ctx->stream;
  const uint32_t n0 = (uint32_t)cloud->n;
  const size_t n1 = std::max<size_t>(n0, 1);
  // every temporary, once: a fit's buffers for n0 points, the other half of the points' double buffer, both halves of the
  // original indices, the labels, the remainder's size
  FitBufs B;
  hipError_t e = fit_alloc(tmp, st, n0, (uint32_t)p.max_iterations + 1u, false, 0, false, B);
  float4 *pts_cur = B.pts_o, *pts_nxt = (float4 *)tmp.get(16 * n1, e);
  int32_t *orig_cur = (int32_t *)tmp.get(4 * n1, e), *orig_nxt = (int32_t *)tmp.get(4 * n1, e);
  int32_t *d_label = label ? (int32_t *)tmp.get(4 * n1, e) : nullptr;
  uint32_t *d_m = (uint32_t *)tmp.get(16, e);
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  if (n0)
    STAGE_LAUNCH(ctx, ctx->plane_stats.launches, pl_peel_init_kernel, 8.0 * n0, dim3(grid_of(n0, kPlBlock)), dim3(kPlBlock), 0, st, n0, orig_cur, d_label);
  uint32_t m = n0;
  int32_t n_planes = 0, stop = OPE_PEEL_FRACTION;
  // objectsegmentationplane.cpp:300-319.  The host knows m from the round's second synchronisation; no cloud is built per round.
  while ((double)m > q.keep_fraction * (double)n0) {
    if (q.max_planes > 0 && n_planes >= q.max_planes) { stop = OPE_PEEL_MAX_PLANES; break; }
    PeelStep step{pts_nxt, orig_cur, orig_nxt, d_label, n_planes, d_m, m};
    Fit fit;
    B.pts_o = pts_cur;
    const int rc = fit_run(ctx, who, B, n_planes == 0 ? cloud : nullptr, m, p, nullptr, 0, nullptr, &step, fit);
    if (rc != OPE_OK) return rc;
    if (!fit.found || fit.n_in == 0) { stop = OPE_PEEL_NO_INLIERS; break; }   // (:308-312; nothing was flagged: this half still holds the remainder)
    if ((size_t)n_planes < cap_planes) {
      if (coeffs) std::memcpy(coeffs + 4 * (size_t)n_planes, fit.coeff, 16);
      if (counts) counts[n_planes] = (int32_t)fit.n_in;
      if (iterations) iterations[n_planes] = ctx->plane_stats.iterations;
    }
    ++n_planes;
    if (step.m_next != m - fit.n_in) return set_err(ctx, OPE_EHIP, std::string(who) + "the remainder's size on the device and the inlier count disagree");
    m = step.m_next;
    std::swap(pts_cur, pts_nxt);
    std::swap(orig_cur, orig_nxt);
  }
  // the remainder as indices, the labels, and the one cloud of the call
  if ((rest_idx && m) || (label && n0)) {
    if (rest_idx && m) e = hipMemcpyAsync(rest_idx, orig_cur, 4ull * m, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && label && n0) e = hipMemcpyAsync(label, d_label, 4ull * n0, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    ++ctx->plane_stats.host_syncs;
    if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  }
  if (rest) {
    const int rc = select_counted(ctx, cloud, orig_cur, m, rest);
    if (rc != OPE_OK) return rc;
  }
  out->n_planes = n_planes;
  out->n_rest = (int32_t)m;
  out->stop = stop;
  out->launches = ctx->plane_stats.launches;
  out->host_syncs = ctx->plane_stats.host_syncs;
  return OPE_OK;
}

int ope_plane_last_stats(const ope_ctx *ctx, ope_plane_stats *out) {
  if (!ctx || !out) return OPE_EINVAL;
  *out = ctx->plane_stats;
  return OPE_OK;
}

int ope_plane_last_hypotheses(const ope_ctx *ctx, int32_t *samples, float *coeffs, int32_t *counts, size_t cap, size_t *n_out) {
  if (!ctx || !n_out) return OPE_EINVAL;
  const size_t made = ctx->plane_counts.size(), w = std::min(made, cap);
  if (samples && w) std::memcpy(samples, ctx->plane_samples.data(), 12 * w);
  if (coeffs && w) std::memcpy(coeffs, ctx->plane_coeffs.data(), 16 * w);
  if (counts && w) std::memcpy(counts, ctx->plane_counts.data(), 4 * w);
  *n_out = made;
  return OPE_OK;
}

int ope_prism_extract(ope_ctx *ctx, const ope_cloud *cloud, const float *hull, size_t m, double height_min, double height_max,
                      int32_t *out_idx, size_t *n_out, ope_cloud **out, float hull_coeff[4]) {
  static const char *who = "ope_prism_extract: ";
  if (!ctx) return OPE_EINVAL;
  ctx->plane_stats = ope_plane_stats{};
  ctx->plane_stats.best = -1;
  if (out) *out = nullptr;
  if (!cloud || !hull || !n_out) return set_err(ctx, OPE_EINVAL, std::string(who) + "bad argument");
  if (m < 3 || m > 65535) return set_err(ctx, OPE_EINVAL, std::string(who) + "a hull has 3 .. 65535 vertices");
  if (cloud->n > (size_t)0x7fffffff) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than 2^31 - 1 points");
  *n_out = 0;
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  TraceRange r(ctx, "prism_extract");
  CallTmp tmp{ctx->stream, {}};
  const uint32_t n = (uint32_t)cloud->n;
  hipError_t e = hipSuccess;
  auto *pts_o = (float4 *)tmp.get(16 * std::max<size_t>(n, 1), e);
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  STAGE_LAUNCH(ctx, ctx->plane_stats.launches, pl_orig_kernel, 32.0 * n, dim3(grid_of(n, kPlBlock)), dim3(kPlBlock), 0, ctx->stream, cloud->view(), pts_o,
               (int32_t *)nullptr);
  int32_t *d_idx = nullptr;
  uint32_t count = 0;
  int rc = prism_run(ctx, tmp, who, cloud, pts_o, hull, m, height_min, height_max, &d_idx, &count, out_idx, hull_coeff);
  if (rc != OPE_OK) return rc;
  *n_out = count;
  if (out) rc = select_counted(ctx, cloud, d_idx, count, out);
  return rc;
}

int ope_tabletop_segment(ope_ctx *ctx, const ope_cloud *cloud, const ope_plane_params *params, ope_tabletop_result *out,
                         ope_cloud **plane, ope_cloud **not_plane, int32_t *prism_idx, int32_t *plane_idx, int32_t *not_plane_idx) {
  static const char *who = "ope_tabletop_segment: ";
  if (!ctx) return OPE_EINVAL;
  ctx->plane_stats = ope_plane_stats{};
  ctx->plane_stats.best = -1;
  if (plane) *plane = nullptr;
  if (not_plane) *not_plane = nullptr;
  if (!cloud || !out || !plane || !not_plane) return set_err(ctx, OPE_EINVAL, std::string(who) + "bad argument");
  ope_plane_params p;
  { const int rc = check_plane_params(ctx, who, params, p); if (rc != OPE_OK) return rc; }
  if (cloud->n > (size_t)0x7fffffff) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than 2^31 - 1 points");
  std::memset(out, 0, sizeof *out);
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  TraceRange r(ctx, "tabletop_segment");
  CallTmp tmp{ctx->stream, {}};
  const hipStream_t st = ctx->stream;
  auto finish = [&](int status) {
    out->status = status;
    out->launches = ctx->plane_stats.launches;
    out->host_syncs = ctx->plane_stats.host_syncs;
    return OPE_OK;
  };
  // 2. the first fit (objectsegmentationplane.cpp:154)
  Fit f1;
  int rc = plane_fit(ctx, tmp, who, cloud, p, nullptr, 0, nullptr, f1);
  if (rc != OPE_OK) return rc;
  out->iterations_first = ctx->plane_stats.iterations;
  if (!f1.found) return finish(OPE_TABLETOP_NO_PLANE_FIRST);
  std::memcpy(out->coeff_first, f1.coeff, 16);
  // 3-4. the inliers projected into the plane, their extreme x and y (getMinMax3D of their hull, :163-172)
  hipError_t e = hipSuccess;
  auto *d_mm = (uint32_t *)tmp.get(16, e);
  uint32_t mm[4] = {0xffffffffu, 0xffffffffu, 0u, 0u};
  if (e == hipSuccess) { e = h2d_copy(st, d_mm, mm, 16); ++ctx->plane_stats.launches; }
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  STAGE_LAUNCH(ctx, ctx->plane_stats.launches, pl_project_minmax_kernel, 20.0 * f1.n_in, dim3(grid_of(f1.n_in, kPlBlock)), dim3(kPlBlock), 0, st, f1.d_pts_o,
               f1.d_idx, f1.n_in, f1.d_coeff, d_mm);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(mm, d_mm, 16, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  ++ctx->plane_stats.host_syncs;
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  // (no inlier: getMinMax3D leaves FLT_MAX / -FLT_MAX)
  const bool any = mm[0] != 0xffffffffu;
  const float min_x = any ? unkey_host(mm[0]) : FLT_MAX, min_y = any ? unkey_host(mm[1]) : FLT_MAX;
  const float max_x = any ? unkey_host(mm[2]) : -FLT_MAX, max_y = any ? unkey_host(mm[3]) : -FLT_MAX;
  // the four corners (:174-188): a double subtraction rounded into a std::vector<float>, z from the plane in float
  const float vx[4] = {(float)(min_x - 0.1), (float)(min_x - 0.1), (float)(max_x + 0.1), (float)(max_x + 0.1)};
  const float vy[4] = {(float)(min_y - 0.1), (float)(max_y + 0.1), (float)(max_y + 0.1), (float)(min_y - 0.1)};
  const float a = f1.coeff[0], b = f1.coeff[1], c = f1.coeff[2], d = f1.coeff[3];
  for (int i = 0; i < 4; ++i) {
    const float x = vx[i], y = vy[i];
    const float z = -((a * x) + (b * y) + d) / c;
    out->corners[3 * i] = x; out->corners[3 * i + 1] = y; out->corners[3 * i + 2] = z;
  }
  // 5. the prism (:210-214) and cloudObjWithPlane (:217-223)
  int32_t *d_pidx = nullptr;
  uint32_t n_prism = 0;
  rc = prism_run(ctx, tmp, who, cloud, f1.d_pts_o, out->corners, 4, 0.0, (double)FLT_MAX, &d_pidx, &n_prism, prism_idx, nullptr);
  if (rc != OPE_OK) return rc;
  out->n_prism = (int32_t)n_prism;
  ope_cloud *with_plane = nullptr;
  rc = select_counted(ctx, cloud, d_pidx, n_prism, &with_plane);
  if (rc != OPE_OK) return rc;
  // 6. the second fit (:227), a new SACSegmentation run: the same seed
  Fit f2;
  rc = plane_fit(ctx, tmp, who, with_plane, p, nullptr, 0, nullptr, f2);
  out->iterations_second = ctx->plane_stats.iterations;
  if (rc != OPE_OK || !f2.found) {
    ope_cloud_free(with_plane);
    return rc != OPE_OK ? rc : finish(OPE_TABLETOP_NO_PLANE_SECOND);
  }
  std::memcpy(out->coeff_second, f2.coeff, 16);
  out->n_plane = (int32_t)f2.n_in;
  out->n_not_plane = (int32_t)(n_prism - f2.n_in);
  // 7. plane and non-plane cloud (:234), and their points as indices into the input
  rc = select_counted(ctx, with_plane, f2.d_idx, f2.n_in, plane);
  if (rc == OPE_OK) rc = select_counted(ctx, with_plane, f2.d_rest, n_prism - f2.n_in, not_plane);
  if (rc == OPE_OK && (plane_idx || not_plane_idx)) {
    auto *d_map = (int32_t *)tmp.get(4 * std::max<size_t>(n_prism, 1), e);
    if (e == hipSuccess && plane_idx) {
      STAGE_LAUNCH(ctx, ctx->plane_stats.launches, pl_compose_kernel, 12.0 * f2.n_in, dim3(grid_of(f2.n_in, kPlBlock)), dim3(kPlBlock), 0, st, d_pidx, f2.d_idx,
                   f2.n_in, d_map);
      if (f2.n_in) e = hipMemcpyAsync(plane_idx, d_map, 4ull * f2.n_in, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess && not_plane_idx) {
      const uint32_t nr = n_prism - f2.n_in;
      STAGE_LAUNCH(ctx, ctx->plane_stats.launches, pl_compose_kernel, 12.0 * nr, dim3(grid_of(nr, kPlBlock)), dim3(kPlBlock), 0, st, d_pidx, f2.d_rest, nr,
                   d_map);
      if (nr) e = hipMemcpyAsync(not_plane_idx, d_map, 4ull * nr, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    ++ctx->plane_stats.host_syncs;
    if (e != hipSuccess) rc = set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  }
  ope_cloud_free(with_plane);
  if (rc != OPE_OK) {
    if (*plane) { ope_cloud_free(*plane); *plane = nullptr; }
    if (*not_plane) { ope_cloud_free(*not_plane); *not_plane = nullptr; }
    return rc;
  }
  return finish(OPE_TABLETOP_OK);
}

}  // extern "C"
