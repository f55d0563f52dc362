// vfh.hip — the reference's object recognition (BuildModel/src/objectdetection.cpp; gfx950, wave64): one Viewpoint Feature
// Histogram (pcl::VFHEstimation::computeFeature, PCL 1.7.x, the defaults: normalize_bins_ on, normalize_distances_ and
// size_component_ off, 45 + 45 + 45 + 45 + 128 bins) per candidate cluster, for every cluster of a frame in one call, and the
// chi-square k nearest rows of a table of trained signatures (FLANN's ChiSquareDistance, exact search).
//
// ope_vfh_batch / ope_vfh_recognise run these launches whatever the number of clusters and their sizes:
//   0. vfh_scatter_kernel     one lane per point: every cloud's points and normals into its ORIGINAL order (uploaded clouds lie
//                             along the Morton curve, w = original index); counts non-finite normals;
//   1. vfh_centroid_kernel    one workgroup per cluster: compute3DCentroid and the mean normal, sequential fp32 sums in the
//                             cloud's order (lanes 0-2 the coordinates, 3-5 the normal), then d_vp_p = viewpoint - centroid,
//                             normalised as a 4-vector;
//   2. vfh_bins_kernel        one lane per point: computePairFeatures(centroid, mean normal, point, normal), the four bins, a
//                             per-workgroup LDS histogram of 308 integers flushed with integer atomics;
//   3. vfh_signature_kernel   one workgroup per cluster, one lane per bin: the float bin PCL ends with, count additions of
//                             hist_incr replayed in order;
//   4. vfh_chi2_kernel        (recognise / match) one workgroup per query: all m distances to a scratch row, then k rounds of a
//                             block arg-min by (distance, index).
// One synchronisation at the end.  Clouds without normals get ope_normals(k, viewpoint 0) first, one call (and one
// synchronisation) per such cloud: that part grows with the clusters.
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "coarse_stages.hpp"
#include "feature_math.hpp"
#include "stage_host.hpp"

struct ope_vfh_db {
  ope_ctx *ctx = nullptr;
  size_t m = 0;
  float *d_cols = nullptr;   // 308 x m: dimension d of row r at d * m + r (the lanes of the distance kernel read along r)
};

namespace ope {
namespace {

constexpr int kVfhBlock = 256;
constexpr int kVfhBins = 308;
constexpr int kVfhSigBlock = 320;   // five waves: one lane per bin
constexpr int kVfhMaxK = 16;
constexpr uint32_t kVfhVpOff = 180;   // 45 + 45 + 45 + 45 (the f4 block stays zero under the defaults)

struct VfhSeg {
  CloudView c;
};

// per cluster: the two centroids and the normalised viewpoint direction
struct VfhGeo {
  float4 cen;   // xyz_centroid
  float4 ncen;  // normal_centroid (not normalised)
  float4 dvp;   // d_vp_p, all four components
};

struct VfhGiven {
  float vp[3];
  int use_centroid;
  float centroid[3];
  int use_normal;
  float normal[3];
};

// 0. original order.  words[0] counts non-finite normals.
__global__ __launch_bounds__(kVfhBlock) void vfh_scatter_kernel(const VfhSeg *__restrict__ segs, const uint32_t *__restrict__ off, uint32_t nseg,
                                                                uint32_t total, float4 *__restrict__ pts, float4 *__restrict__ nrm,
                                                                uint32_t *__restrict__ words) {
  const uint32_t p = blockIdx.x * kVfhBlock + threadIdx.x;
  if (p >= total) return;
  const uint32_t s = seg_of(off, nseg, p), b = off[s], n = off[s + 1] - b;
  const float4 q = segs[s].c.xyzw[p - b];
  const float4 v = segs[s].c.nrm[p - b];
  const uint32_t o = (uint32_t)__float_as_int(q.w);
  if (o >= n) return;   // (not a cloud's index: never for a cloud the library made)
  pts[(size_t)b + o] = make_float4(q.x, q.y, q.z, 1.f);
  nrm[(size_t)b + o] = make_float4(v.x, v.y, v.z, 0.f);
  if (!(isfinite(v.x) && isfinite(v.y) && isfinite(v.z))) atomicAdd(&words[0], 1u);
}

// 1. the centroids.  Lane d < 3 adds coordinate d of every point in the cloud's order, lane 3 + d component d of its normal.
__global__ __launch_bounds__(kVfhBlock) void vfh_centroid_kernel(const uint32_t *__restrict__ off, const float4 *__restrict__ pts,
                                                                 const float4 *__restrict__ nrm, VfhGiven g, VfhGeo *__restrict__ geo) {
  __shared__ float s_v[6][kVfhBlock];
  __shared__ float s_sum[6];
  const uint32_t s = blockIdx.x, b = off[s], n = off[s + 1] - b, t = threadIdx.x;
  float acc = 0.f;
  for (uint32_t base = 0; base < n; base += kVfhBlock) {
    const uint32_t m = min((uint32_t)kVfhBlock, n - base);
    if (t < m) {
      const float4 q = pts[(size_t)b + base + t], v = nrm[(size_t)b + base + t];
      s_v[0][t] = q.x; s_v[1][t] = q.y; s_v[2][t] = q.z;
      s_v[3][t] = v.x; s_v[4][t] = v.y; s_v[5][t] = v.z;
    }
    __syncthreads();
    if (t < 6)
      for (uint32_t j = 0; j < m; ++j) acc = __fadd_rn(acc, s_v[t][j]);
    __syncthreads();
  }
  if (t < 6) s_sum[t] = acc;
  __syncthreads();
  if (t != 0) return;
  VfhGeo r;
  const float fn = (float)n;
  // compute3DCentroid: centroid /= n, then w = 1; an empty cloud keeps zeros (its row is never binned).  setCentroidToUse takes
  // a Vector3f: w = 0.
  float cw = 1.f;
  if (g.use_centroid) { r.cen = make_float4(g.centroid[0], g.centroid[1], g.centroid[2], 0.f); cw = 0.f; }
  else if (n > 0) r.cen = make_float4(__fdiv_rn(s_sum[0], fn), __fdiv_rn(s_sum[1], fn), __fdiv_rn(s_sum[2], fn), 1.f);
  else r.cen = make_float4(0.f, 0.f, 0.f, 1.f);
  if (g.use_normal) r.ncen = make_float4(g.normal[0], g.normal[1], g.normal[2], 0.f);
  else if (n > 0) r.ncen = make_float4(__fdiv_rn(s_sum[3], fn), __fdiv_rn(s_sum[4], fn), __fdiv_rn(s_sum[5], fn), 0.f);
  else r.ncen = make_float4(0.f, 0.f, 0.f, 0.f);
  // d_vp_p = Vector4f(vp, 0) - xyz_centroid; d_vp_p.normalize(): squared norm summed x, y, z, w, each component divided
  const float dx = __fsub_rn(g.vp[0], r.cen.x), dy = __fsub_rn(g.vp[1], r.cen.y), dz = __fsub_rn(g.vp[2], r.cen.z), dw = __fsub_rn(0.f, cw);
  const float sq = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)), __fmul_rn(dw, dw));
  const float nv = __fsqrt_rn(sq);
  r.dvp = make_float4(__fdiv_rn(dx, nv), __fdiv_rn(dy, nv), __fdiv_rn(dz, nv), __fdiv_rn(dw, nv));
  geo[s] = r;
}

__device__ __forceinline__ int vfh_bin_angle(float f1) {
  const double d_pi = (double)(1.0f / (2.0f * 3.14159274f));
  const int h = (int)floor(45 * (((double)f1 + 3.14159265358979323846) * d_pi));
  return min(max(h, 0), 44);
}
__device__ __forceinline__ int vfh_bin_unit(float f) {
  const int h = (int)floor(45 * (((double)f + 1.0) * 0.5));
  return min(max(h, 0), 44);
}

// 2. the bins.  A workgroup's LDS histogram belongs to the cluster of its first point; lanes of another cluster (a workgroup that
// straddles a boundary) add to the global counts directly.  Integer counts: the result does not depend on the order of the adds.
// words[1] counts rejected pairs.
__global__ __launch_bounds__(kVfhBlock) void vfh_bins_kernel(const uint32_t *__restrict__ off, uint32_t nseg, uint32_t total,
                                                             const float4 *__restrict__ pts, const float4 *__restrict__ nrm,
                                                             const VfhGeo *__restrict__ geo, int32_t *__restrict__ counts,
                                                             uchar4 *__restrict__ bins_out, uint32_t *__restrict__ words) {
  __shared__ int s_hist[kVfhBins];
  const uint32_t first = blockIdx.x * kVfhBlock, p = first + threadIdx.x;
  for (int i = threadIdx.x; i < kVfhBins; i += kVfhBlock) s_hist[i] = 0;
  const uint32_t s0 = seg_of(off, nseg, first);   // (first < total for every launched block)
  __syncthreads();
  if (p < total) {
    const uint32_t s = seg_of(off, nseg, p);
    const VfhGeo g = geo[s];
    const float4 q = pts[p], v = nrm[p];
    float f1 = 0.f, f2 = 0.f, f3 = 0.f;
    const bool ok = pair_features(g.cen.x, g.cen.y, g.cen.z, g.ncen.x, g.ncen.y, g.ncen.z, q.x, q.y, q.z, v.x, v.y, v.z, f1, f2, f3);
    // alpha = (normal.dot(d_vp_p) + 1.0) * 0.5 with normal = (nx, ny, nz, 0): the dot in float, x y z w; the rest in double
    const float dot = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(v.x, g.dvp.x), __fmul_rn(v.y, g.dvp.y)), __fmul_rn(v.z, g.dvp.z)),
                                __fmul_rn(0.f, g.dvp.w));
    const double alpha = ((double)dot + 1.0) * 0.5;
    int bv = (int)floor(alpha * 128.0);
    bv = min(max(bv, 0), 127);
    int b1 = 0xFF, b2 = 0xFF, b3 = 0xFF;
    if (ok) { b1 = vfh_bin_angle(f1); b2 = vfh_bin_unit(f2); b3 = vfh_bin_unit(f3); }
    else atomicAdd(&words[1], 1u);
    if (s == s0) {
      if (ok) { atomicAdd(&s_hist[b1], 1); atomicAdd(&s_hist[45 + b2], 1); atomicAdd(&s_hist[90 + b3], 1); }
      atomicAdd(&s_hist[kVfhVpOff + bv], 1);
    } else {
      int32_t *c = counts + (size_t)s * kVfhBins;
      if (ok) { atomicAdd(&c[b1], 1); atomicAdd(&c[45 + b2], 1); atomicAdd(&c[90 + b3], 1); }
      atomicAdd(&c[kVfhVpOff + bv], 1);
    }
    if (bins_out) bins_out[p] = make_uchar4((unsigned char)b1, (unsigned char)b2, (unsigned char)b3, (unsigned char)bv);
  }
  __syncthreads();
  int32_t *c0 = counts + (size_t)s0 * kVfhBins;
  for (int i = threadIdx.x; i < kVfhBins; i += kVfhBlock) {
    const int h = s_hist[i];
    if (h) atomicAdd(&c0[i], h);
  }
}

// 3. the signature.  PCL adds hist_incr to a float bin once per hit: count sequential additions from 0, not count * incr.
// f1..f3: hist_incr = 100.0f / (float)(n - 1) (n = 1: +inf, and every pair of such a cloud is rejected); the viewpoint block:
// (float)(100.0 / (double)n).  The f4 block adds hist_incr_size_component = 0: it stays 0.
__global__ __launch_bounds__(kVfhSigBlock) void vfh_signature_kernel(const uint32_t *__restrict__ off, const int32_t *__restrict__ counts,
                                                                     float *__restrict__ sig) {
  const uint32_t s = blockIdx.x, n = off[s + 1] - off[s], t = threadIdx.x;
  if (t >= kVfhBins) return;
  float h = 0.f;
  if (n > 0 && (t < 135 || t >= kVfhVpOff)) {
    const float incr = t < 135 ? __fdiv_rn(100.0f, (float)(n - 1)) : (float)(100.0 / (double)n);
    const uint32_t c = min((uint32_t)counts[(size_t)s * kVfhBins + t], n);   // (a count never exceeds the cluster's size)
    for (uint32_t j = 0; j < c; ++j) h = __fadd_rn(h, incr);
  }
  sig[(size_t)s * kVfhBins + t] = h;
}

// 4. chi-square k nearest rows.  flann::ChiSquareDistance: per dimension in order, s = a + b; if (s > 0) r += (a - b)^2 / s.
// out_idx / out_dist (q x k): -1 / +inf past m.  Ties go to the lower row.
__global__ __launch_bounds__(kVfhBlock) void vfh_chi2_kernel(const float *__restrict__ cols, uint32_t m, const float *__restrict__ queries, int k,
                                                             float *__restrict__ dist, int32_t *__restrict__ out_idx,
                                                             float *__restrict__ out_dist) {
  __shared__ float s_q[kVfhBins];
  __shared__ float s_d[kVfhBlock];
  __shared__ int s_i[kVfhBlock];
  const uint32_t qi = blockIdx.x, t = threadIdx.x;
  for (int i = t; i < kVfhBins; i += kVfhBlock) s_q[i] = queries[(size_t)qi * kVfhBins + i];
  __syncthreads();
  float *row = dist + (size_t)qi * m;
  for (uint32_t r = t; r < m; r += kVfhBlock) {
    float acc = 0.f;
    for (int d = 0; d < kVfhBins; ++d) {
      const float a = s_q[d], b = cols[(size_t)d * m + r];
      const float sum = __fadd_rn(a, b);
      if (sum > 0.f) {
        const float diff = __fsub_rn(a, b);
        acc = __fadd_rn(acc, __fdiv_rn(__fmul_rn(diff, diff), sum));
      }
    }
    row[r] = acc;
  }
  __syncthreads();
  float pd = -INFINITY;   // the pair taken in the round before: the next one is the smallest pair above it
  int pi = -1;
  for (int round = 0; round < k; ++round) {
    float bd = INFINITY;
    int bi = -1;
    for (uint32_t r = t; r < m; r += kVfhBlock) {
      const float d = row[r];
      const bool after = pi < 0 || d > pd || (d == pd && (int)r > pi);
      if (after && (bi < 0 || d < bd)) { bd = d; bi = (int)r; }   // (r ascends: an equal distance keeps the lower row)
    }
    s_d[t] = bd; s_i[t] = bi;
    __syncthreads();
    for (int w = kVfhBlock / 2; w > 0; w >>= 1) {
      if ((int)t < w) {
        const float od = s_d[t + w];
        const int oi = s_i[t + w];
        if (oi >= 0 && (s_i[t] < 0 || od < s_d[t] || (od == s_d[t] && oi < s_i[t]))) { s_d[t] = od; s_i[t] = oi; }
      }
      __syncthreads();
    }
    pd = s_d[0]; pi = s_i[0];
    __syncthreads();
    if (t == 0) {
      out_idx[(size_t)qi * k + round] = pi;
      out_dist[(size_t)qi * k + round] = pi >= 0 ? pd : INFINITY;
    }
    if (pi < 0) {   // the table is exhausted (uniform: every lane read the same s_i[0])
      if (t == 0)
        for (int r2 = round + 1; r2 < k; ++r2) { out_idx[(size_t)qi * k + r2] = -1; out_dist[(size_t)qi * k + r2] = INFINITY; }
      break;
    }
  }
}

bool finite3(const float *v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// the refusals of the VFH stages, before anything is launched
int vfh_check(ope_ctx *ctx, const std::string &who, size_t n, ope_cloud *const *clusters, const ope_vfh_params &p) {
  if (n == 0 || !clusters) return set_err(ctx, OPE_EINVAL, who + "bad argument");
  if (n > 65535) return set_err(ctx, OPE_EINVAL, who + "more than 65535 clusters");
  if (p.normals_k < 3 || p.normals_k > 32) return set_err(ctx, OPE_EINVAL, who + "3 <= normals_k <= 32");
  if (!finite3(p.viewpoint)) return set_err(ctx, OPE_EINVAL, who + "viewpoint must be finite");
  if (p.use_given_centroid && !finite3(p.centroid)) return set_err(ctx, OPE_EINVAL, who + "centroid must be finite");
  if (p.use_given_normal && !finite3(p.normal)) return set_err(ctx, OPE_EINVAL, who + "normal must be finite");
  if (p.use_given_centroid && std::memcmp(p.centroid, p.viewpoint, 12) == 0)
    return set_err(ctx, OPE_EINVAL, who + "the given centroid is the viewpoint: PCL normalises a zero vector there");
  uint64_t total = 0;
  for (size_t i = 0; i < n; ++i) {
    const ope_cloud *c = clusters[i];
    const std::string at = " (cluster " + std::to_string(i) + ")";
    if (!c) return set_err(ctx, OPE_EINVAL, who + "no cluster cloud" + at);
    if (c->n_valid != c->n) return set_err(ctx, OPE_EINVAL, who + "the cloud has non-finite points: PCL's bin of a NaN is undefined" + at);
    if (c->d_nrm && c->nrm_nonfinite == 1)
      return set_err(ctx, OPE_EINVAL, who + "the cloud has non-finite normals: PCL's bin of a NaN is undefined" + at);
    total += c->n;
    if (total > 0x7fffffffull) return set_err(ctx, OPE_EINVAL, who + "more than 2^31-1 points in all");
  }
  return OPE_OK;
}

int match_check(ope_ctx *ctx, const std::string &who, const ope_vfh_db *db, size_t q, int k) {
  if (!db) return set_err(ctx, OPE_EINVAL, who + "no table");
  if (db->m == 0) return set_err(ctx, OPE_EINVAL, who + "the table is empty");
  if (k < 1 || k > kVfhMaxK) return set_err(ctx, OPE_EINVAL, who + "1 <= k <= 16");
  if (q == 0) return set_err(ctx, OPE_EINVAL, who + "no queries");
  if (db->m > 0x7fffffffull) return set_err(ctx, OPE_EINVAL, who + "more than 2^31-1 rows");
  return OPE_OK;
}

// stage 4 on device queries; the outputs stay on the device
int match_enqueue(ope_ctx *ctx, CallTmp &tmp, const ope_vfh_db *db, const float *d_queries, size_t q, int k, int32_t **d_idx, float **d_dist) {
  hipError_t e = hipSuccess;
  auto *dist = (float *)tmp.get(4ull * q * db->m, e);
  *d_idx = (int32_t *)tmp.get(4ull * q * (size_t)k, e);
  *d_dist = (float *)tmp.get(4ull * q * (size_t)k, e);
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string("ope_vfh_match: buffers: ") + hipGetErrorString(e));
  STAGE_LAUNCH(ctx, ctx->vfh_stats.launches, vfh_chi2_kernel, (double)q * (4.0 * kVfhBins * (double)db->m + 4.0 * kVfhBins), dim3((unsigned)q), dim3(kVfhBlock),
               0, ctx->stream, db->d_cols, (uint32_t)db->m, d_queries, k, dist, *d_idx, *d_dist);
  return OPE_OK;
}

// stages 0-3 of n checked clusters; the signatures stay at *d_sig (n x 308).  Nothing is waited for.
int vfh_enqueue(ope_ctx *ctx, CallTmp &tmp, const std::string &who, size_t n, ope_cloud *const *clusters, const ope_vfh_params &p,
                bool want_bins, float **d_sig, int32_t **d_counts, uchar4 **d_bins, uint32_t **d_words, uint32_t *total_out) {
  // the normals: each cloud's own, or ope_normals' (left on the cloud)
  for (size_t i = 0; i < n; ++i)
    if (!clusters[i]->d_nrm && clusters[i]->n > 0) {
      const int rc = ope_normals(ctx, clusters[i], p.normals_k, nullptr, nullptr, nullptr);
      if (rc != OPE_OK) return rc;
      ++ctx->vfh_stats.normals_estimated;
      ++ctx->vfh_stats.host_syncs;
    }
  // one block: the segments, then the offsets
  std::vector<unsigned char> head(sizeof(VfhSeg) * n + 4 * (n + 1));
  auto *segs = (VfhSeg *)head.data();
  std::vector<uint32_t> off(n + 1, 0);
  for (size_t i = 0; i < n; ++i) {
    segs[i].c = clusters[i]->view();
    off[i + 1] = off[i] + (uint32_t)clusters[i]->n;
    if (clusters[i]->n == 0) ++ctx->vfh_stats.empty_clouds;
  }
  std::memcpy(head.data() + sizeof(VfhSeg) * n, off.data(), 4 * (n + 1));
  const uint32_t total = off[n];
  *total_out = total;
  ctx->vfh_stats.points = total;
  const hipStream_t st = ctx->stream;
  hipError_t e = hipSuccess;
  auto *d_head = (unsigned char *)tmp.get(head.size(), e);
  auto *pts = (float4 *)tmp.get(16ull * std::max<uint32_t>(total, 1), e);
  auto *nrm = (float4 *)tmp.get(16ull * std::max<uint32_t>(total, 1), e);
  auto *geo = (VfhGeo *)tmp.get(sizeof(VfhGeo) * n, e);
  *d_counts = (int32_t *)tmp.get(4ull * kVfhBins * n, e);
  *d_sig = (float *)tmp.get(4ull * kVfhBins * n, e);
  *d_bins = want_bins ? (uchar4 *)tmp.get(4ull * std::max<uint32_t>(total, 1), e) : nullptr;
  *d_words = (uint32_t *)tmp.get(16, e);
  if (e == hipSuccess) e = h2d_copy(st, d_head, head.data(), head.size(), &ctx->vfh_stats.host_syncs);   // (a staged upload waits: beyond ~100 clusters)
  if (e == hipSuccess) e = hipMemsetAsync(*d_counts, 0, 4ull * kVfhBins * n, st);
  if (e == hipSuccess) e = hipMemsetAsync(*d_words, 0, 16, st);
  ctx->vfh_stats.launches += 2;
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, who + "buffers: " + hipGetErrorString(e));
  const auto *d_segs = (const VfhSeg *)d_head;
  const auto *d_off = (const uint32_t *)(d_head + sizeof(VfhSeg) * n);
  VfhGiven g{};
  std::memcpy(g.vp, p.viewpoint, 12);
  g.use_centroid = p.use_given_centroid != 0;
  std::memcpy(g.centroid, p.centroid, 12);
  g.use_normal = p.use_given_normal != 0;
  std::memcpy(g.normal, p.normal, 12);
  const unsigned pblocks = (total + kVfhBlock - 1) / kVfhBlock;
  TraceRange r(ctx, "vfh");
  if (total)
    STAGE_LAUNCH(ctx, ctx->vfh_stats.launches, vfh_scatter_kernel, 64.0 * total, dim3(pblocks), dim3(kVfhBlock), 0, st, d_segs, d_off, (uint32_t)n, total, pts,
                 nrm, *d_words);
  STAGE_LAUNCH(ctx, ctx->vfh_stats.launches, vfh_centroid_kernel, 32.0 * total, dim3((unsigned)n), dim3(kVfhBlock), 0, st, d_off, pts, nrm, g, geo);
  if (total)
    STAGE_LAUNCH(ctx, ctx->vfh_stats.launches, vfh_bins_kernel, 36.0 * total, dim3(pblocks), dim3(kVfhBlock), 0, st, d_off, (uint32_t)n, total, pts, nrm, geo,
                 *d_counts, *d_bins, *d_words);
  STAGE_LAUNCH(ctx, ctx->vfh_stats.launches, vfh_signature_kernel, 8.0 * kVfhBins * n, dim3((unsigned)n), dim3(kVfhSigBlock), 0, st, d_off, *d_counts, *d_sig);
  return OPE_OK;
}

// the end of a call: the copies back, the one synchronisation, the verdict on the normals
int vfh_finish(ope_ctx *ctx, const std::string &who, hipError_t e, const uint32_t *d_words) {
  uint32_t words[4] = {0, 0, 0, 0};
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess && d_words) e = hipMemcpyAsync(words, d_words, 16, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  ++ctx->vfh_stats.host_syncs;
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, who + hipGetErrorString(e));
  ctx->vfh_stats.rejected_pairs = words[1];
  if (words[0])   // (normals the host never saw: estimated or gathered on the device)
    return set_err(ctx, OPE_EINVAL, who + std::to_string(words[0]) + " normal(s) are not finite: PCL's bin of a NaN is undefined");
  return OPE_OK;
}

}  // namespace
}  // namespace ope

using namespace ope;

extern "C" {

void ope_vfh_default_params(ope_vfh_params *p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->normals_k = 30;   // objectdetection.cpp:17
}

int ope_vfh_batch(ope_ctx *ctx, size_t n, ope_cloud *const *clusters, const ope_vfh_params *params, float *out308, int32_t *counts_opt,
                  unsigned char *bins_opt) {
  const std::string who = "ope_vfh_batch: ";
  if (!ctx) return OPE_EINVAL;
  ctx->vfh_stats = ope_vfh_stats{};
  if (!out308) return set_err(ctx, OPE_EINVAL, who + "bad argument");
  ope_vfh_params p;
  if (params) p = *params; else ope_vfh_default_params(&p);
  int rc = vfh_check(ctx, who, n, clusters, p);
  if (rc != OPE_OK) return rc;
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  CallTmp tmp{ctx->stream};
  float *d_sig; int32_t *d_counts; uchar4 *d_bins; uint32_t *d_words; uint32_t total = 0;
  rc = vfh_enqueue(ctx, tmp, who, n, clusters, p, bins_opt != nullptr, &d_sig, &d_counts, &d_bins, &d_words, &total);
  if (rc != OPE_OK) return rc;
  hipError_t e = hipMemcpyAsync(out308, d_sig, 4ull * kVfhBins * n, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && counts_opt) e = hipMemcpyAsync(counts_opt, d_counts, 4ull * kVfhBins * n, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && bins_opt && total) e = hipMemcpyAsync(bins_opt, d_bins, 4ull * total, hipMemcpyDeviceToHost, ctx->stream);
  return vfh_finish(ctx, who, e, d_words);
}

int ope_vfh_last_stats(const ope_ctx *ctx, ope_vfh_stats *out) {
  if (!ctx || !out) return OPE_EINVAL;
  *out = ctx->vfh_stats;
  return OPE_OK;
}

int ope_vfh_db_create(ope_ctx *ctx, const float *rows, size_t m, ope_vfh_db **db) {
  const std::string who = "ope_vfh_db_create: ";
  if (!ctx) return OPE_EINVAL;
  if (!db) return set_err(ctx, OPE_EINVAL, who + "bad argument");
  *db = nullptr;
  if (!rows || m == 0) return set_err(ctx, OPE_EINVAL, who + "an empty table");
  if (m > 0x7fffffffull / kVfhBins) return set_err(ctx, OPE_EINVAL, who + "too many rows");
  std::vector<float> cols((size_t)kVfhBins * m);
  for (size_t r = 0; r < m; ++r)
    for (int d = 0; d < kVfhBins; ++d) {
      const float v = rows[r * kVfhBins + d];
      if (!std::isfinite(v)) return set_err(ctx, OPE_EINVAL, who + "row " + std::to_string(r) + " is not finite");
      cols[(size_t)d * m + r] = v;
    }
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  auto *t = new ope_vfh_db;
  t->ctx = ctx;
  t->m = m;
  hipError_t e = hipMalloc((void **)&t->d_cols, 4ull * kVfhBins * m);
  if (e == hipSuccess) e = h2d_copy(ctx->stream, t->d_cols, cols.data(), 4ull * kVfhBins * m);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    if (t->d_cols) (void)hipFree(t->d_cols);
    delete t;
    return set_err(ctx, OPE_EHIP, who + hipGetErrorString(e));
  }
  *db = t;
  return OPE_OK;
}

void ope_vfh_db_free(ope_vfh_db *db) {
  if (!db) return;
  if (db->d_cols) (void)hipFree(db->d_cols);
  delete db;
}

size_t ope_vfh_db_size(const ope_vfh_db *db) { return db ? db->m : 0; }

int ope_vfh_match(ope_ctx *ctx, const ope_vfh_db *db, const float *queries308, size_t q, int k, int32_t *out_idx, float *out_dist) {
  const std::string who = "ope_vfh_match: ";
  if (!ctx) return OPE_EINVAL;
  ctx->vfh_stats = ope_vfh_stats{};
  if (!queries308 || !out_idx || !out_dist) return set_err(ctx, OPE_EINVAL, who + "bad argument");
  int rc = match_check(ctx, who, db, q, k);
  if (rc != OPE_OK) return rc;
  for (size_t i = 0; i < q * kVfhBins; ++i)
    if (!std::isfinite(queries308[i])) return set_err(ctx, OPE_EINVAL, who + "query " + std::to_string(i / kVfhBins) + " is not finite");
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  CallTmp tmp{ctx->stream};
  hipError_t e = hipSuccess;
  auto *d_q = (float *)tmp.get(4ull * kVfhBins * q, e);
  if (e == hipSuccess) e = h2d_copy(ctx->stream, d_q, queries308, 4ull * kVfhBins * q);
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, who + hipGetErrorString(e));
  int32_t *d_idx; float *d_dist;
  rc = match_enqueue(ctx, tmp, db, d_q, q, k, &d_idx, &d_dist);
  if (rc != OPE_OK) return rc;
  e = hipMemcpyAsync(out_idx, d_idx, 4ull * q * k, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out_dist, d_dist, 4ull * q * k, hipMemcpyDeviceToHost, ctx->stream);
  return vfh_finish(ctx, who, e, nullptr);
}

int ope_vfh_recognise(ope_ctx *ctx, const ope_vfh_db *db, size_t n, ope_cloud *const *clusters, const ope_vfh_params *params, int k,
                      float *out308_opt, int32_t *out_idx, float *out_dist) {
  const std::string who = "ope_vfh_recognise: ";
  if (!ctx) return OPE_EINVAL;
  ctx->vfh_stats = ope_vfh_stats{};
  if (!out_idx || !out_dist) return set_err(ctx, OPE_EINVAL, who + "bad argument");
  ope_vfh_params p;
  if (params) p = *params; else ope_vfh_default_params(&p);
  int rc = vfh_check(ctx, who, n, clusters, p);
  if (rc == OPE_OK) rc = match_check(ctx, who, db, n, k);
  if (rc != OPE_OK) return rc;
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  CallTmp tmp{ctx->stream};
  float *d_sig; int32_t *d_counts; uchar4 *d_bins; uint32_t *d_words; uint32_t total = 0;
  rc = vfh_enqueue(ctx, tmp, who, n, clusters, p, false, &d_sig, &d_counts, &d_bins, &d_words, &total);
  if (rc != OPE_OK) return rc;
  int32_t *d_idx; float *d_dist;
  rc = match_enqueue(ctx, tmp, db, d_sig, n, k, &d_idx, &d_dist);
  if (rc != OPE_OK) return rc;
  hipError_t e = hipMemcpyAsync(out_idx, d_idx, 4ull * n * k, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out_dist, d_dist, 4ull * n * k, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && out308_opt) e = hipMemcpyAsync(out308_opt, d_sig, 4ull * kVfhBins * n, hipMemcpyDeviceToHost, ctx->stream);
  return vfh_finish(ctx, who, e, d_words);
}

}  // extern "C"
