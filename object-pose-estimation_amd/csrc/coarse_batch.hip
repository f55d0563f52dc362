// coarse_batch.hip — the reference's coarse stage (estimateCoarsePose, poseestimator.cpp:16-73) for one model and many candidate
// clusters in one call (ope_coarse_pose_batch, gfx950, wave64).
//
// The single path (ope_uniform_sampling, ope_normals, ope_fpfh, ope_index_build, ope_sacia) runs one cloud at a time, builds an
// index per neighbourhood query and synchronises the host several times per cloud, on clouds of a few hundred key points.  Here
// every stage runs once for all clouds ("segments": the model, then the clusters):
//   1. uniform sampling: voxel keys per segment, ONE segmented radix sort, PCL's survivor rule per voxel run, one scan that packs
//      the key points of all segments;
//   2. normals: one workgroup per (segment, tile of 256 queries), the segment's key points staged in LDS, a brute-force ascending
//      k-list in registers, then the covariance and eigen code of normals_kernel itself (feature_math.hpp);
//   3. FPFH: the same staging, brute-force radius neighbours, the SPFH and the 1/d^2-weighted pass of spfh_kernel / fpfh_kernel;
//   4. SAC-IA: the host draws and fits of ope_sacia (sacia_draws, umeyama_host), one feature-kNN launch over (query, cluster) and
//      one error launch over (hypothesis, cluster), the cluster's key points in LDS, sums in a fixed order per hypothesis.
// Neither the launches nor the host synchronisations depend on the number of clusters, and nothing is summed across clusters,
// so a cluster's result does not depend on the rest of the batch.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "coarse_stages.hpp"
#include "feature_math.hpp"
#include "stage_host.hpp"

namespace ope {

constexpr int kIdxBits = 17;        // original index < 65536 in 17 bits: no valid key has all its low bits set
constexpr int kKeyBits = kIdxBits + 31;   // voxel < 2^31 (PCL's int leaf index): every valid key fits 48 bits
constexpr int kListK = kKnnMaxK;    // register k-list length (k <= 32 is used)
constexpr int kSpfhRow = 36;        // 33 bins padded, as in features.hip

// 1a. key = voxel << 17 | original index (voxel_key_kernel per segment); non-finite points ~0, last in their segment
__global__ __launch_bounds__(kCoarseBlock) void coarse_voxel_key_kernel(const CoarseSeg *__restrict__ segs, const uint32_t *__restrict__ off,
                                                                          uint32_t nseg, uint32_t total, unsigned long long *__restrict__ keys,
                                                                          uint32_t *__restrict__ vals) {
  const uint32_t p = blockIdx.x * kCoarseBlock + threadIdx.x;
  if (p >= total) return;
  const uint32_t s = seg_of(off, nseg, p);
  const CoarseSeg g = segs[s];
  const uint32_t i = p - off[s];
  vals[p] = i;
  if (i >= g.c.n_valid) { keys[p] = ~0ull; return; }
  const float4 q = g.c.xyzw[i];
  const int ix = (int)floorf(q.x * g.inv_leaf) - g.min_b[0], iy = (int)floorf(q.y * g.inv_leaf) - g.min_b[1],
            iz = (int)floorf(q.z * g.inv_leaf) - g.min_b[2];
  const unsigned long long voxel = (unsigned long long)ix + (unsigned long long)iy * g.div_x + (unsigned long long)iz * g.div_xy;
  keys[p] = (voxel << kIdxBits) | (unsigned long long)(uint32_t)__float_as_int(q.w);
}

// 1b. the head of every voxel run walks its run: PCL's survivor is the minimum of (distance to the voxel's integer corner, position)
// (voxel_min_kernel's rule); win = the survivor's position in its cloud, flag = 1 at heads.  flags has total + 1 entries.
__global__ __launch_bounds__(kCoarseBlock) void coarse_voxel_pick_kernel(const CoarseSeg *__restrict__ segs, const uint32_t *__restrict__ off,
                                                                           uint32_t nseg, uint32_t total, const unsigned long long *__restrict__ keys,
                                                                           const uint32_t *__restrict__ vals, uint32_t *__restrict__ win,
                                                                           uint32_t *__restrict__ flags) {
  const uint32_t p = blockIdx.x * kCoarseBlock + threadIdx.x;
  if (p == total) flags[p] = 0u;
  if (p >= total) return;
  const uint32_t s = seg_of(off, nseg, p);
  const unsigned long long k = keys[p];
  const unsigned long long vox = k >> kIdxBits;
  const bool head = k != ~0ull && (p == off[s] || (keys[p - 1] >> kIdxBits) != vox);
  flags[p] = head ? 1u : 0u;
  if (!head) return;
  const CoarseSeg g = segs[s];
  const uint32_t end = off[s + 1];
  unsigned long long best = ~0ull;
  for (uint32_t r = p; r < end && keys[r] != ~0ull && (keys[r] >> kIdxBits) == vox; ++r) {
    const float4 q = g.c.xyzw[vals[r]];
    const float ix = floorf(q.x * g.inv_leaf), iy = floorf(q.y * g.inv_leaf), iz = floorf(q.z * g.inv_leaf);
    const float d = (q.x - ix) * (q.x - ix) + (q.y - iy) * (q.y - iy) + (q.z - iz) * (q.z - iz) + 1.0f;
    const unsigned long long m = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)r;
    best = m < best ? m : best;
  }
  win[p] = vals[(uint32_t)(best & 0xffffffffull)];
}

// 1c. pack the survivors: kp[slot] = the key point (w = its original index); key_off[s] = first slot of segment s (nseg + 1 entries)
__global__ __launch_bounds__(kCoarseBlock) void coarse_key_pack_kernel(const CoarseSeg *__restrict__ segs, const uint32_t *__restrict__ off,
                                                                         uint32_t nseg, uint32_t total, const uint32_t *__restrict__ win,
                                                                         const uint32_t *__restrict__ flags, const uint32_t *__restrict__ slot,
                                                                         float4 *__restrict__ kp, uint32_t *__restrict__ key_off) {
  const uint32_t p = blockIdx.x * kCoarseBlock + threadIdx.x;
  if (p <= nseg) key_off[p] = slot[off[p]];
  if (p >= total || !flags[p]) return;
  kp[slot[p]] = segs[seg_of(off, nseg, p)].c.xyzw[win[p]];
}

// one workgroup per tile: (segment, first query); the segment's key points are kp[key_off[s] .. key_off[s + 1])
__device__ __forceinline__ void tile_of(const int2 *__restrict__ tiles, const uint32_t *__restrict__ key_off, uint32_t &s0, uint32_t &m,
                                        uint32_t &q) {
  const int2 t = tiles[blockIdx.x];
  s0 = key_off[t.x];
  m = key_off[t.x + 1] - s0;
  q = (uint32_t)t.y + threadIdx.x;
}

// 2. NormalEstimation (k-NN, self included) of every key point against its own segment.  The list is kept ascending with strict
// comparisons (an equal earlier candidate stays in front), the neighbours are accumulated in list order, as normals_kernel does.
__global__ __launch_bounds__(kCoarseBlock) void coarse_normals_kernel(const float4 *__restrict__ kp, const uint32_t *__restrict__ key_off,
                                                                        const int2 *__restrict__ tiles, int k, float vpx, float vpy, float vpz,
                                                                        float4 *__restrict__ out_nrm) {
  extern __shared__ float4 s_pts[];
  uint32_t s0, m, q;
  tile_of(tiles, key_off, s0, m, q);
  for (uint32_t j = threadIdx.x; j < m; j += kCoarseBlock) s_pts[j] = kp[s0 + j];
  __syncthreads();
  const bool on = q < m;
  const float4 s = on ? s_pts[q] : make_float4(0.f, 0.f, 0.f, 0.f);
  float d[kListK];
  uint32_t pi[kListK];
#pragma unroll
  for (int j = 0; j < kListK; ++j) { d[j] = on ? INFINITY : -INFINITY; pi[j] = 0; }
  for (uint32_t t = 0; t < m; ++t) {
    const float4 P = s_pts[t];
    const float dist = sq_dist3(__fsub_rn(s.x, P.x), __fsub_rn(s.y, P.y), __fsub_rn(s.z, P.z));
    const bool ins = dist < d[kListK - 1];
    if (__ballot(ins) == 0ull) continue;
    // sorted insert (KnnRegVisitor): new d[j] = median(d[j-1], d[j], dist)
    bool lt_hi = ins;
#pragma unroll
    for (int j = kListK - 1; j > 0; --j) {
      const bool lt_lo = dist < d[j - 1];
      pi[j] = lt_lo ? pi[j - 1] : (lt_hi ? t : pi[j]);
      d[j] = __builtin_amdgcn_fmed3f(d[j - 1], d[j], dist);
      lt_hi = lt_lo;
    }
    pi[0] = lt_hi ? t : pi[0];
    d[0] = lt_hi ? dist : d[0];
  }
  if (!on) return;
  const int count = (int)min((uint32_t)k, m);
  const float qnan = __int_as_float(0x7fc00000);
  if (count < 3) { out_nrm[s0 + q] = make_float4(qnan, qnan, qnan, qnan); return; }
  float accu[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < kListK; ++j)
    if (j < count) { const float4 p = s_pts[pi[j]]; OPE_ACCUMULATE_NEIGHBOUR(p); }
  out_nrm[s0 + q] = normal_from_sums(accu, count, s, vpx, vpy, vpz);
}

// 3a. SPFH of every key point (spfh_kernel's arithmetic): every segment point within r, self (the same slot) excluded from the pairs
__global__ __launch_bounds__(kCoarseBlock) void coarse_spfh_kernel(const float4 *__restrict__ kp, const float4 *__restrict__ nrm,
                                                                     const uint32_t *__restrict__ key_off, const int2 *__restrict__ tiles,
                                                                     float r2, float *__restrict__ spfh) {
  extern __shared__ float4 s_dyn4[];
  __shared__ unsigned short s_hist[33][kCoarseBlock];   // (a segment holds at most OPE_COARSE_MAX_KEYS points: counts fit 16 bits)
  uint32_t s0, m, q;
  tile_of(tiles, key_off, s0, m, q);
  float4 *s_pts = s_dyn4, *s_nrm = s_dyn4 + m;
  for (uint32_t j = threadIdx.x; j < m; j += kCoarseBlock) { s_pts[j] = kp[s0 + j]; s_nrm[j] = nrm[s0 + j]; }
  __syncthreads();
  if (q >= m) return;
  unsigned short *hist = &s_hist[0][threadIdx.x];
#pragma unroll
  for (int b = 0; b < 33; ++b) hist[b * kCoarseBlock] = 0;
  const float4 s = s_pts[q], n = s_nrm[q];
  int cnt = 0;
  for (uint32_t t = 0; t < m; ++t) {
    const float4 P = s_pts[t];
    const float dist = sq_dist3(__fsub_rn(s.x, P.x), __fsub_rn(s.y, P.y), __fsub_rn(s.z, P.z));
    if (!(dist <= r2)) continue;
    ++cnt;
    if (t == q) continue;
    const float4 nj = s_nrm[t];
    float f1, f2, f3;
    if (!pair_features(s.x, s.y, s.z, n.x, n.y, n.z, P.x, P.y, P.z, nj.x, nj.y, nj.z, f1, f2, f3)) continue;
    hist[spfh_bin_angle(f1) * kCoarseBlock] += 1;
    hist[(11 + spfh_bin_unit(f2)) * kCoarseBlock] += 1;
    hist[(22 + spfh_bin_unit(f3)) * kCoarseBlock] += 1;
  }
  const float hist_incr = 100.0f / (float)(cnt - 1);
  float *row = spfh + (size_t)(s0 + q) * kSpfhRow;
#pragma unroll
  for (int b = 0; b < 33; ++b) {
    const uint32_t c = hist[b * kCoarseBlock];
    float h = 0.f;
    for (uint32_t a = 0; a < c; ++a) h = __fadd_rn(h, hist_incr);
    row[b] = h;
  }
}

// 3b. FPFH (fpfh_kernel's arithmetic): the 1/d^2-weighted SPFH rows of the neighbours within r, self excluded, in slot order
__global__ __launch_bounds__(kCoarseBlock) void coarse_fpfh_kernel(const float4 *__restrict__ kp, const uint32_t *__restrict__ key_off,
                                                                     const int2 *__restrict__ tiles, float r2, const float *__restrict__ spfh,
                                                                     float *__restrict__ out33) {
  extern __shared__ float4 s_pts[];
  uint32_t s0, m, q;
  tile_of(tiles, key_off, s0, m, q);
  for (uint32_t j = threadIdx.x; j < m; j += kCoarseBlock) s_pts[j] = kp[s0 + j];
  __syncthreads();
  if (q >= m) return;
  const float4 s = s_pts[q];
  float acc[33];
#pragma unroll
  for (int b = 0; b < 33; ++b) acc[b] = 0.f;
  double sum0 = 0.0, sum1 = 0.0, sum2 = 0.0;
  int cnt = 0;
  for (uint32_t t = 0; t < m; ++t) {
    const float4 P = s_pts[t];
    const float dist = sq_dist3(__fsub_rn(s.x, P.x), __fsub_rn(s.y, P.y), __fsub_rn(s.z, P.z));
    if (!(dist <= r2)) continue;
    ++cnt;
    if (dist == 0.f) continue;
    const float w = 1.0f / dist;
    const float *row = spfh + (size_t)(s0 + t) * kSpfhRow;
#pragma unroll
    for (int b = 0; b < 11; ++b) { const float val = row[b] * w; sum0 += (double)val; acc[b] += val; }
#pragma unroll
    for (int b = 11; b < 22; ++b) { const float val = row[b] * w; sum1 += (double)val; acc[b] += val; }
#pragma unroll
    for (int b = 22; b < 33; ++b) { const float val = row[b] * w; sum2 += (double)val; acc[b] += val; }
  }
  float *o = out33 + (size_t)(s0 + q) * 33;
  if (cnt == 0) {
    for (int b = 0; b < 33; ++b) o[b] = __int_as_float(0x7fc00000);
    return;
  }
  const double k0 = sum0 != 0 ? 100.0 / sum0 : 0.0, k1 = sum1 != 0 ? 100.0 / sum1 : 0.0, k2 = sum2 != 0 ? 100.0 / sum2 : 0.0;
#pragma unroll
  for (int b = 0; b < 11; ++b) o[b] = acc[b] * (float)k0;
#pragma unroll
  for (int b = 11; b < 22; ++b) o[b] = acc[b] * (float)k1;
#pragma unroll
  for (int b = 22; b < 33; ++b) o[b] = acc[b] * (float)k2;
}

// 4a. findSimilarFeatures: block (u, c) = the u-th distinct model sample of active cluster c against that cluster's descriptors
__global__ __launch_bounds__(256) void coarse_feature_knn_kernel(const float *__restrict__ fpfh, const uint32_t *__restrict__ key_off,
                                                                  const int2 *__restrict__ active, const int32_t *__restrict__ uniq,
                                                                  int max_uniq, int k, int32_t *__restrict__ out_idx) {
  const int2 a = active[blockIdx.y];   // (segment, distinct samples)
  if ((int)blockIdx.x >= a.y) return;
  const size_t u = (size_t)blockIdx.y * max_uniq + blockIdx.x;
  const uint32_t t0 = key_off[a.x], nt = key_off[a.x + 1] - t0;
  feature_knn_block(fpfh + (size_t)t0 * 33, (int)nt, fpfh + (size_t)(key_off[0] + (uint32_t)uniq[u]) * 33, k, out_idx + u * k);
}

// 4b. computeErrorMetric: block (h, c) = hypothesis h of active cluster c; every model key point's truncated squared 1-NN distance
// to the cluster's key points (LDS, brute force), summed in a fixed order: per lane, then wave_sum, then the four waves in turn
__global__ __launch_bounds__(256) void coarse_sacia_error_kernel(const float4 *__restrict__ kp, const uint32_t *__restrict__ key_off,
                                                                  const int2 *__restrict__ active, const float *__restrict__ T_rows,
                                                                  float thr, double *__restrict__ err_out) {
  extern __shared__ float4 s_pts[];
  __shared__ double s_red[4];
  const int2 a = active[blockIdx.y];
  const uint32_t t0 = key_off[a.x], nt = key_off[a.x + 1] - t0, ns = key_off[1] - key_off[0];
  for (uint32_t j = threadIdx.x; j < nt; j += 256) s_pts[j] = kp[t0 + j];
  __syncthreads();
  const size_t hyp = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  const float *F = T_rows + 12 * hyp;
  double err = 0.0;
  for (uint32_t i = threadIdx.x; i < ns; i += 256) {
    const float4 s = kp[key_off[0] + i];
    const float x = xform_row(F + 0, s.x, s.y, s.z);
    const float y = xform_row(F + 4, s.x, s.y, s.z);
    const float z = xform_row(F + 8, s.x, s.y, s.z);
    float best = INFINITY;
    for (uint32_t t = 0; t < nt; ++t) {
      const float4 P = s_pts[t];
      best = fminf(best, sq_dist3(__fsub_rn(x, P.x), __fsub_rn(y, P.y), __fsub_rn(z, P.z)));
    }
    err += (double)((best <= thr) ? best / thr : 1.0f);
  }
  const double w = wave_sum(err);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) err_out[hyp] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

// a key point's original index (the bits of w)
static int32_t orig_index(const float4 &q) {
  int32_t i;
  std::memcpy(&i, &q.w, 4);
  return i;
}

long long host_key_count(const ope_cloud *c, float inv) {
  if (c->n_valid == 0) return 0;
  long long min_b[3], div_b[3];
  for (int d = 0; d < 3; ++d) {
    min_b[d] = (long long)std::floor(c->bb_lo[d] * inv);
    div_b[d] = (long long)std::floor(c->bb_hi[d] * inv) - min_b[d] + 1;
  }
  if ((double)div_b[0] * (double)div_b[1] * (double)div_b[2] >= 2147483648.0) return -1;
  std::vector<unsigned long long> v;
  v.reserve(c->n_valid);
  const float *xyz = c->h_xyz.data();
  for (size_t i = 0; i < c->n; ++i) {
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    if (!(std::isfinite(x) && std::isfinite(y) && std::isfinite(z))) continue;
    const long long ix = (long long)std::floor(x * inv) - min_b[0], iy = (long long)std::floor(y * inv) - min_b[1],
                    iz = (long long)std::floor(z * inv) - min_b[2];
    v.push_back((unsigned long long)(ix + iy * div_b[0] + iz * div_b[0] * div_b[1]));
  }
  std::sort(v.begin(), v.end());
  return (long long)(std::unique(v.begin(), v.end()) - v.begin());
}

hipError_t coarse_sample_segments(ope_ctx *ctx, CallTmp &tmp, const CoarseSeg *d_segs, const uint32_t *d_off, size_t nseg, uint32_t total,
                                  float4 **d_kp_out, uint32_t **d_key_off_out, std::vector<uint32_t> &key_off, const char *&what,
                                  const void *d_extra, void *h_extra, size_t extra_bytes) {
  hipError_t e = hipSuccess;
  what = "buffers";
  const uint32_t nt1 = total + 1;
  auto *d_keys = (unsigned long long *)tmp.get(8 * (size_t)nt1, e);
  auto *d_keys2 = (unsigned long long *)tmp.get(8 * (size_t)nt1, e);
  auto *d_vals = (uint32_t *)tmp.get(4 * (size_t)nt1, e);
  auto *d_vals2 = (uint32_t *)tmp.get(4 * (size_t)nt1, e);
  auto *d_win = (uint32_t *)tmp.get(4 * (size_t)nt1, e);
  auto *d_flags = (uint32_t *)tmp.get(4 * (size_t)nt1, e);
  auto *d_slot = (uint32_t *)tmp.get(4 * (size_t)nt1, e);
  auto *d_kp = (float4 *)tmp.get(16 * (size_t)nt1, e);
  auto *d_key_off = (uint32_t *)tmp.get(4 * (nseg + 1), e);
  if (e != hipSuccess) return e;
  *d_kp_out = d_kp;
  *d_key_off_out = d_key_off;
  key_off.assign(nseg + 1, 0);
  TraceRange r(ctx, "coarse_uniform_sampling");
  what = "uniform sampling";
  const unsigned nb = (unsigned)((std::max(total, (uint32_t)nseg) + kCoarseBlock) / kCoarseBlock);
  size_t tb_sort = 0, tb_scan = 0;
  e = rocprim::segmented_radix_sort_pairs(nullptr, tb_sort, d_keys, d_keys2, d_vals, d_vals2, total, (unsigned)nseg, d_off, d_off + 1, 0,
                                          kKeyBits, ctx->stream);
  if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, tb_scan, d_flags, d_slot, 0u, (size_t)nt1, rocprim::plus<uint32_t>(), ctx->stream);
  size_t tb = std::max(tb_sort, tb_scan);
  void *d_tmp = tmp.get(tb, e);
  if (e != hipSuccess) return e;
  {
    KernelTimer kt(ctx, "coarse_voxel_key_kernel", 28.0 * total);
    if (total) hipLaunchKernelGGL(coarse_voxel_key_kernel, dim3(nb), dim3(kCoarseBlock), 0, ctx->stream, d_segs, d_off, (uint32_t)nseg, total,
                                  d_keys, d_vals);
  }
  what = "segmented sort";
  if (total) e = rocprim::segmented_radix_sort_pairs(d_tmp, tb, d_keys, d_keys2, d_vals, d_vals2, total, (unsigned)nseg, d_off, d_off + 1, 0,
                                                     kKeyBits, ctx->stream);
  if (e != hipSuccess) return e;
  STAGE_LAUNCH_TIMED(ctx, coarse_voxel_pick_kernel, "coarse_voxel_pick_kernel", 40.0 * total, dim3(nb), dim3(kCoarseBlock), 0, ctx->stream, d_segs, d_off,
                     (uint32_t)nseg, total, d_keys2, d_vals2, d_win, d_flags);
  what = "scan";
  tb = std::max(tb_sort, tb_scan);
  e = rocprim::exclusive_scan(d_tmp, tb, d_flags, d_slot, 0u, (size_t)nt1, rocprim::plus<uint32_t>(), ctx->stream);
  if (e != hipSuccess) return e;
  STAGE_LAUNCH_TIMED(ctx, coarse_key_pack_kernel, "coarse_key_pack_kernel", 28.0 * total, dim3(nb), dim3(kCoarseBlock), 0, ctx->stream, d_segs, d_off,
                     (uint32_t)nseg, total, d_win, d_flags, d_slot, d_kp, d_key_off);
  what = "uniform sampling";
  e = hipMemcpyAsync(key_off.data(), d_key_off, 4 * (nseg + 1), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && extra_bytes) e = hipMemcpyAsync(h_extra, d_extra, extra_bytes, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  return e;
}

hipError_t coarse_normals_launch(ope_ctx *ctx, const float4 *d_kp, const uint32_t *d_key_off, const int2 *d_tiles, size_t n_tiles,
                                 uint32_t nkeys, uint32_t max_keys, int k, const float vp[3], float4 *d_nrm) {
  if (n_tiles == 0) return hipSuccess;
  const size_t lds = 16 * (size_t)max_keys;
  const hipError_t e = hipFuncSetAttribute((const void *)coarse_normals_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  KernelTimer kt(ctx, "coarse_normals_kernel", (double)nkeys * (12.0 + 12.0 * k + 16.0));
  hipLaunchKernelGGL(coarse_normals_kernel, dim3((unsigned)n_tiles), dim3(kCoarseBlock), lds, ctx->stream, d_kp, d_key_off, d_tiles, k, vp[0],
                     vp[1], vp[2], d_nrm);
  return hipGetLastError();
}

}  // namespace ope

using namespace ope;

extern "C" {

void ope_coarse_default_params(ope_coarse_params *p) {
  if (!p) return;
  p->key_leaf = 0.01f;
  p->normals_k = 30;
  p->viewpoint[0] = p->viewpoint[1] = p->viewpoint[2] = 0.f;
  p->fpfh_radius = 0.03f;
  ope_sacia_default_params(&p->sacia);
}

int ope_coarse_pose_batch(ope_ctx *ctx, const ope_cloud *model, size_t n, const ope_cloud *const *clusters,
                          const ope_coarse_params *params, const uint64_t *seeds, ope_coarse_batch_result *out) {
  return coarse_pose_batch_impl(ctx, model, n, clusters, params, seeds, false, out, nullptr);
}

}  // extern "C"

// ope_coarse_pose_batch's refusals (n >= 1, clusters not NULL checked by the caller), before anything is launched: parameters,
// sizes, and the key points of every cloud that could exceed the cap.  *model_keys = the model's key points.
int ope::coarse_batch_check(ope_ctx *ctx, const ope_cloud *model, size_t n, const ope_cloud *const *clusters, const ope_coarse_params &p,
                            long long *model_keys, const char *who) {
  const int S = p.sacia.nr_samples, K = p.sacia.k_correspondences, H = p.sacia.max_iterations;
  if (!(p.key_leaf > 0) || !(p.fpfh_radius > 0)) return set_err(ctx, OPE_EINVAL, std::string(who) + "key_leaf and fpfh_radius must be > 0");
  if (p.normals_k < 1 || p.normals_k > kKnnMaxK) return set_err(ctx, OPE_EINVAL, std::string(who) + "1 <= normals_k <= 32");
  if (K < 1 || K > kFeatK) return set_err(ctx, OPE_EINVAL, std::string(who) + "1 <= k_correspondences <= 8");
  if (S < 1 || H < 1) return set_err(ctx, OPE_EINVAL, std::string(who) + "nr_samples and max_iterations must be >= 1");
  for (size_t i = 0; i < n; ++i)
    if (!clusters[i]) return set_err(ctx, OPE_EINVAL, std::string(who) + "no cluster cloud (cluster " + std::to_string(i) + ")");

  // ---- refusals, before anything is launched: sizes, and the key points of every cloud that could exceed the cap
  const size_t nseg = n + 1;
  const float inv = 1.0f / p.key_leaf;
  auto cloud_of = [&](size_t s) { return s == 0 ? model : clusters[s - 1]; };
  long long mk = -2;
  for (size_t s = 0; s < nseg; ++s) {
    const ope_cloud *c = cloud_of(s);
    const std::string at = s == 0 ? std::string(" (model)") : " (cluster " + std::to_string(s - 1) + ")";
    if (c->n > (size_t)OPE_COARSE_MAX_POINTS)
      return set_err(ctx, OPE_EINVAL, std::string(who) + "more than OPE_COARSE_MAX_POINTS points" + at);
    { const int rch = c->ensure_host(); if (rch != OPE_OK) return rch; }
    if (s == 0 || c->n_valid > (size_t)OPE_COARSE_MAX_KEYS) {
      const long long kc = host_key_count(c, inv);
      if (kc < 0) return set_err(ctx, OPE_EINVAL, std::string(who) + "leaf size too small for the input dataset" + at);
      if (kc > OPE_COARSE_MAX_KEYS) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than OPE_COARSE_MAX_KEYS key points" + at);
      if (s == 0) mk = kc;
    } else if (c->n_valid > 0 && host_key_count(c, inv) < 0) {
      return set_err(ctx, OPE_EINVAL, std::string(who) + "leaf size too small for the input dataset" + at);
    }
  }
  if (mk < S) return set_err(ctx, OPE_EINVAL, std::string(who) + "the model has fewer key points than nr_samples");
  if (model_keys) *model_keys = mk;
  return OPE_OK;
}

// Steps 1-3 for the model (segment 0) and the n clusters, enqueued: uniform sampling (one synchronisation: the key offsets), then
// the normals and FPFH launches.  model_keys = coarse_batch_check's count.
int ope::coarse_front_launch(ope_ctx *ctx, CallTmp &tmp, const char *who, const ope_cloud *model, size_t n, const ope_cloud *const *clusters,
                             const ope_coarse_params &p, long long model_keys, CoarseFront &f) {
  const size_t nseg = n + 1;
  const float inv = 1.0f / p.key_leaf;
  auto cloud_of = [&](size_t s) { return s == 0 ? model : clusters[s - 1]; };
  std::vector<CoarseSeg> segs(nseg);
  std::vector<uint32_t> off(nseg + 1, 0);
  for (size_t s = 0; s < nseg; ++s) {
    const ope_cloud *c = cloud_of(s);
    CoarseSeg &g = segs[s];
    g.c = c->view();
    g.inv_leaf = inv;
    long long min_b[3] = {0, 0, 0}, div_b[3] = {1, 1, 1};
    if (c->n_valid > 0)
      for (int d = 0; d < 3; ++d) {
        min_b[d] = (long long)std::floor(c->bb_lo[d] * inv);
        div_b[d] = (long long)std::floor(c->bb_hi[d] * inv) - min_b[d] + 1;
      }
    for (int d = 0; d < 3; ++d) g.min_b[d] = (int)min_b[d];
    g.div_x = (uint32_t)div_b[0];
    g.div_xy = (uint32_t)(div_b[0] * div_b[1]);
    off[s + 1] = off[s] + (uint32_t)c->n;
  }
  const uint32_t total = off[nseg];

  hipError_t e = hipSuccess;
  auto fail = [&](const char *what) { return set_err(ctx, OPE_EHIP, std::string(who) + what + ": " + hipGetErrorString(e)); };
  auto *d_segs = (CoarseSeg *)tmp.get(sizeof(CoarseSeg) * nseg, e);
  auto *d_off = (uint32_t *)tmp.get(4 * (nseg + 1), e);
  if (e == hipSuccess) e = h2d_copy(ctx->stream, d_segs, segs.data(), sizeof(CoarseSeg) * nseg);
  if (e == hipSuccess) e = h2d_copy(ctx->stream, d_off, off.data(), 4 * (nseg + 1));
  if (e != hipSuccess) return fail("buffers");

  // ---- 1. uniform sampling of all segments
  std::vector<uint32_t> &key_off = f.key_off;
  float4 *d_kp = nullptr;
  uint32_t *d_key_off = nullptr;
  {
    const char *what = "";
    e = coarse_sample_segments(ctx, tmp, d_segs, d_off, nseg, total, &d_kp, &d_key_off, key_off, what);
    if (e != hipSuccess) return fail(what);
  }
  const uint32_t nkeys = key_off[nseg];
  uint32_t max_keys = 0;
  for (size_t s = 0; s < nseg; ++s) max_keys = std::max(max_keys, key_off[s + 1] - key_off[s]);
  const uint32_t nsk = key_off[1] - key_off[0];
  if ((long long)nsk != model_keys || max_keys > (uint32_t)OPE_COARSE_MAX_KEYS)
    return set_err(ctx, OPE_EHIP, std::string(who) + "key-point count differs from the host count");

  // ---- 2./3. normals and FPFH of every segment's key points
  std::vector<int2> tiles;
  for (size_t s = 0; s < nseg; ++s)
    for (uint32_t q = 0; q < key_off[s + 1] - key_off[s]; q += kCoarseBlock) tiles.push_back(make_int2((int)s, (int)q));
  const size_t nk1 = std::max<size_t>(nkeys, 1);
  auto *d_tiles = (int2 *)tmp.get(sizeof(int2) * std::max<size_t>(tiles.size(), 1), e);
  auto *d_nrm = (float4 *)tmp.get(16 * nk1, e);
  auto *d_spfh = (float *)tmp.get(sizeof(float) * kSpfhRow * nk1, e);
  auto *d_fpfh = (float *)tmp.get(sizeof(float) * 33 * nk1, e);
  if (e == hipSuccess && !tiles.empty()) e = h2d_copy(ctx->stream, d_tiles, tiles.data(), sizeof(int2) * tiles.size());
  if (e != hipSuccess) return fail("buffers");
  const float r2 = p.fpfh_radius * p.fpfh_radius;
  if (!tiles.empty()) {
    const size_t lds1 = 16 * (size_t)max_keys, lds2 = 32 * (size_t)max_keys;
    e = hipFuncSetAttribute((const void *)coarse_spfh_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void *)coarse_fpfh_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1);
    if (e != hipSuccess) return fail("LDS size");
    const dim3 grid((unsigned)tiles.size());
    {
      TraceRange r(ctx, "coarse_normals");
      e = coarse_normals_launch(ctx, d_kp, d_key_off, d_tiles, tiles.size(), nkeys, max_keys, p.normals_k, p.viewpoint, d_nrm);
      if (e != hipSuccess) return fail("LDS size");
    }
    {
      TraceRange r(ctx, "coarse_fpfh");
      KernelTimer kt_s(ctx, "coarse_spfh_kernel", 0.0);
      hipLaunchKernelGGL(coarse_spfh_kernel, grid, dim3(kCoarseBlock), lds2, ctx->stream, d_kp, d_nrm, d_key_off, d_tiles, r2, d_spfh);
      kt_s.stop();
      KernelTimer kt_w(ctx, "coarse_fpfh_kernel", 0.0);
      hipLaunchKernelGGL(coarse_fpfh_kernel, grid, dim3(kCoarseBlock), lds1, ctx->stream, d_kp, d_key_off, d_tiles, r2, d_spfh, d_fpfh);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return fail("features");
  }
  f.nkeys = nkeys; f.max_keys = max_keys; f.nsk = nsk;
  f.d_kp = d_kp; f.d_key_off = d_key_off; f.d_nrm = d_nrm; f.d_fpfh = d_fpfh;
  return OPE_OK;
}

// the key points (xyz, w = original index), normals and FPFH rows of every segment on their way to the host; the caller synchronises
hipError_t ope::coarse_front_download(ope_ctx *ctx, CoarseFront &f) {
  const uint32_t nkeys = f.nkeys;
  hipError_t e = hipSuccess;
  f.h_kp.resize(nkeys);
  if (nkeys) e = hipMemcpyAsync(f.h_kp.data(), f.d_kp, 16 * (size_t)nkeys, hipMemcpyDeviceToHost, ctx->stream);
  f.h_nrm4.resize((size_t)nkeys * 4);
  f.h_fpfh.resize((size_t)nkeys * 33);
  if (e == hipSuccess && nkeys) e = hipMemcpyAsync(f.h_nrm4.data(), f.d_nrm, 16 * (size_t)nkeys, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && nkeys) e = hipMemcpyAsync(f.h_fpfh.data(), f.d_fpfh, sizeof(float) * 33 * (size_t)nkeys, hipMemcpyDeviceToHost, ctx->stream);
  return e;
}

// keep what was computed for ope_coarse_batch_features (after the synchronisation that follows coarse_front_download)
void ope::coarse_front_keep(ope_ctx *ctx, CoarseFront &f) {
  const uint32_t nkeys = f.nkeys;
  ctx->coarse_key_off.assign(f.key_off.begin(), f.key_off.end());
  ctx->coarse_key_idx.resize(nkeys);
  ctx->coarse_nrm.resize((size_t)nkeys * 3);
  for (uint32_t j = 0; j < nkeys; ++j) {
    ctx->coarse_key_idx[j] = orig_index(f.h_kp[j]);
    for (int d = 0; d < 3; ++d) ctx->coarse_nrm[3 * (size_t)j + d] = f.h_nrm4[4 * (size_t)j + d];
  }
  ctx->coarse_fpfh.swap(f.h_fpfh);
}

int ope::coarse_pose_batch_impl(ope_ctx *ctx, const ope_cloud *model, size_t n, const ope_cloud *const *clusters, const ope_coarse_params *params,
                                const uint64_t *seeds, bool seed_by_rank, ope_coarse_batch_result *out, uint64_t *seeds_used) {
  static const char *who = "ope_coarse_pose_batch: ";
  if (!ctx) return set_err(ctx, OPE_EINVAL, "ope_coarse_pose_batch: bad argument");
  if (n == 0) return OPE_OK;
  if (!model || !clusters || !out) return set_err(ctx, OPE_EINVAL, std::string(who) + "bad argument");
  if (n > 65535) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than 65535 clusters (one grid row each)");
  ope_coarse_params p;
  ope_coarse_default_params(&p);
  if (params) p = *params;
  const int S = p.sacia.nr_samples, K = p.sacia.k_correspondences, H = p.sacia.max_iterations;
  long long model_keys = -2;
  { const int rc = coarse_batch_check(ctx, model, n, clusters, p, &model_keys); if (rc != OPE_OK) return rc; }

  OPE_HIP(ctx, hipSetDevice(ctx->device));
  TraceRange r_all(ctx, "coarse_batch");
  CallTmp tmp{ctx->stream, {}};
  hipError_t e = hipSuccess;
  auto fail = [&](const char *what) { return set_err(ctx, OPE_EHIP, std::string(who) + what + ": " + hipGetErrorString(e)); };
  CoarseFront front;
  { const int rc = coarse_front_launch(ctx, tmp, who, model, n, clusters, p, model_keys, front); if (rc != OPE_OK) return rc; }
  const std::vector<uint32_t> &key_off = front.key_off;
  const uint32_t max_keys = front.max_keys, nsk = front.nsk;
  float4 *const d_kp = front.d_kp;
  uint32_t *const d_key_off = front.d_key_off;
  float *const d_fpfh = front.d_fpfh;

  // ---- host: key indices and xyz (the draws need the model's), then the draws while the device computes the features
  e = coarse_front_download(ctx, front);
  if (e != hipSuccess) return fail("download");
  const std::vector<float4> &h_kp = front.h_kp;

  std::vector<int2> active;   // (segment, distinct samples) of every cluster that runs SAC-IA
  std::vector<size_t> active_cluster;
  for (size_t i = 0; i < n; ++i) {
    ope_coarse_batch_result &o = out[i];
    std::memcpy(o.T, kIdentity4, sizeof kIdentity4);
    o.best_error = 0;
    o.best_iteration = -1;
    o.n_src_keys = (int32_t)nsk;
    o.n_tgt_keys = (int32_t)(key_off[i + 2] - key_off[i + 1]);
    o.status = clusters[i]->n == 0 ? OPE_COARSE_EMPTY_TARGET : o.n_tgt_keys < 10 ? OPE_COARSE_FEW_TARGET_FEATURES : OPE_COARSE_OK;
    if (seeds_used) seeds_used[i] = 0;
    if (o.status == OPE_COARSE_OK) { active.push_back(make_int2((int)(i + 1), 0)); active_cluster.push_back(i); }
  }
  const size_t na = active.size();
  std::vector<float> model_xyz((size_t)nsk * 3);
  {
    const float *hx = model->h_xyz.data();
    // (the key points' original indices are only on the host once the copies above are done: the draws read the model's xyz by
    // original index, so they wait for that)
    e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail("download");
    for (uint32_t j = 0; j < nsk; ++j) std::memcpy(&model_xyz[3 * (size_t)j], hx + 3 * (size_t)orig_index(h_kp[j]), 12);
  }
  coarse_front_keep(ctx, front);
  if (na == 0) return OPE_OK;

  // ---- 4. SAC-IA of every active cluster
  TraceRange r_sac(ctx, "coarse_sacia");
  const size_t HS = (size_t)H * S;
  std::vector<std::vector<int32_t>> samp(na, std::vector<int32_t>(HS)), pick(na, std::vector<int32_t>(HS));
  std::vector<std::map<int32_t, int>> slot(na);
  int max_uniq = 0;
  for (size_t a = 0; a < na; ++a) {
    const size_t i = active_cluster[a];
    const uint64_t seed = seeds ? seeds[i] : p.sacia.seed + (uint64_t)(seed_by_rank ? a : i);
    if (seeds_used) seeds_used[i] = seed;
    sacia_draws(model_xyz.data(), (int)nsk, S, K, H, p.sacia.min_sample_dist, seed, samp[a].data(), pick[a].data());
    for (int32_t s : samp[a]) slot[a].emplace(s, (int)slot[a].size());
    active[a].y = (int)slot[a].size();
    max_uniq = std::max(max_uniq, active[a].y);
  }
  std::vector<int32_t> uniq(na * (size_t)max_uniq, 0);
  for (size_t a = 0; a < na; ++a)
    for (const auto &kv : slot[a]) uniq[a * max_uniq + kv.second] = kv.first;
  auto *d_active = (int2 *)tmp.get(sizeof(int2) * na, e);
  auto *d_uniq = (int32_t *)tmp.get(4 * uniq.size(), e);
  auto *d_nn = (int32_t *)tmp.get(4 * uniq.size() * K, e);
  if (e == hipSuccess) e = h2d_copy(ctx->stream, d_active, active.data(), sizeof(int2) * na);
  if (e == hipSuccess) e = h2d_copy(ctx->stream, d_uniq, uniq.data(), 4 * uniq.size());
  if (e != hipSuccess) return fail("buffers");
  std::vector<int32_t> nn(uniq.size() * K);
  STAGE_LAUNCH_TIMED(ctx, coarse_feature_knn_kernel, "coarse_feature_knn_kernel", 132.0 * (double)uniq.size() * (double)max_keys,
                     dim3((unsigned)max_uniq, (unsigned)na), dim3(256), 0, ctx->stream, d_fpfh, d_key_off, d_active, d_uniq, max_uniq, K, d_nn);
  e = hipMemcpyAsync(nn.data(), d_nn, 4 * nn.size(), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return fail("feature knn");

  // one rigid transform per hypothesis (TransformationEstimationSVD), as ope_sacia fits them
  std::vector<float> T(na * (size_t)H * 16), rows(na * (size_t)H * 12), ps((size_t)S * 3), pt((size_t)S * 3);
  for (size_t a = 0; a < na; ++a) {
    const uint32_t t0 = key_off[active[a].x];
    for (int it = 0; it < H; ++it) {
      for (int s = 0; s < S; ++s) {
        const size_t j = (size_t)it * S + s;
        const int32_t *row = &nn[(a * max_uniq + slot[a][samp[a][j]]) * K];
        const int32_t c = row[pick[a][j]] >= 0 ? row[pick[a][j]] : row[0];
        const float4 q = h_kp[t0 + (uint32_t)c];
        std::memcpy(&ps[3 * s], &model_xyz[3 * (size_t)samp[a][j]], 12);
        pt[3 * s] = q.x; pt[3 * s + 1] = q.y; pt[3 * s + 2] = q.z;
      }
      float *Th = &T[(a * H + it) * 16];
      umeyama_host(ps.data(), pt.data(), S, Th);
      colmajor_to_rows12(Th, &rows[(a * H + it) * 12]);
    }
  }
  auto *d_rows = (float *)tmp.get(sizeof(float) * rows.size(), e);
  auto *d_err = (double *)tmp.get(sizeof(double) * na * H, e);
  if (e == hipSuccess) e = h2d_copy(ctx->stream, d_rows, rows.data(), sizeof(float) * rows.size());
  if (e == hipSuccess) e = hipFuncSetAttribute((const void *)coarse_sacia_error_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(16 * max_keys));
  if (e != hipSuccess) return fail("buffers");
  std::vector<double> err(na * (size_t)H);
  STAGE_LAUNCH_TIMED(ctx, coarse_sacia_error_kernel, "coarse_sacia_error_kernel", 16.0 * (double)nsk * (double)H * (double)na, dim3((unsigned)H, (unsigned)na),
                     dim3(256), 16 * (size_t)max_keys, ctx->stream, d_kp, d_key_off, d_active, d_rows, (float)p.sacia.max_corr_dist, d_err);
  e = hipMemcpyAsync(err.data(), d_err, sizeof(double) * err.size(), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return fail("error metric");
  // the reference's "lowest error wins" scan (ope_sacia's), per cluster
  for (size_t a = 0; a < na; ++a) {
    double lowest = 0;
    int best = -1;
    for (int it = 0; it < H; ++it) {
      const double v = err[a * H + it];
      if (it == 0 || (float)v < (float)lowest) { lowest = v; best = it; }
    }
    ope_coarse_batch_result &o = out[active_cluster[a]];
    std::memcpy(o.T, &T[(a * H + best) * 16], sizeof(float) * 16);
    o.best_error = lowest;
    o.best_iteration = best;
  }
  return OPE_OK;
}

extern "C" {

int ope_coarse_batch_features(ope_ctx *ctx, int which, int32_t *key_idx, float *normals, float *fpfh33, size_t cap, size_t *n_out) {
  if (!ctx || !n_out) return set_err(ctx, OPE_EINVAL, "ope_coarse_batch_features: bad argument");
  *n_out = 0;
  const std::vector<int32_t> &off = ctx->coarse_key_off;
  if (off.empty()) return set_err(ctx, OPE_EINVAL, "ope_coarse_batch_features: no ope_coarse_pose_batch call yet");
  const long long s = (long long)which + 1;
  if (s < 0 || s + 1 >= (long long)off.size()) return set_err(ctx, OPE_EINVAL, "ope_coarse_batch_features: `which` out of range");
  const size_t b = (size_t)off[s], m = (size_t)off[s + 1] - b, w = std::min(m, cap);
  if (key_idx) std::memcpy(key_idx, ctx->coarse_key_idx.data() + b, 4 * w);
  if (normals) std::memcpy(normals, ctx->coarse_nrm.data() + 3 * b, 12 * w);
  if (fpfh33) std::memcpy(fpfh33, ctx->coarse_fpfh.data() + 33 * b, 132 * w);
  *n_out = m;
  return OPE_OK;
}

}  // extern "C"
