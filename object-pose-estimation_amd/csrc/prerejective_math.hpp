// prerejective_math.hpp — what ope_prerejective (prerejective.hip) and ope_prerejective_pose_batch (prerejective_batch.hip) share, so
// that the single and the batched call run the same instructions: the host draws, CorrespondenceRejectorPoly's edge test, the fp64
// Umeyama fit of one hypothesis and the sum rule of one (hypothesis, 256 source points) work item.  The callers differ only in
// where a pair comes from: `pair(i, s, t)` hands out the i-th sampled source point and its target point.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <string>

#include "bvh_traverse.hpp"
#include "feature_math.hpp"
#include "icp_update.hpp"

namespace ope {

constexpr int kPrBlock = 256;
constexpr int kPrMaxIterations = 1 << 20;

// the refusals of the parameters, the same for one alignment and for a batch; who: the entry point its errors name
inline int prerej_check_params(ope_ctx *ctx, const char *who, const ope_prerejective_params &p) {
  const auto refuse = [&](const char *why) { return set_err(ctx, OPE_EINVAL, std::string(who) + why); };
  if (p.max_iterations < 1 || p.max_iterations > kPrMaxIterations) return refuse("max_iterations must be 1 .. 2^20");
  if (p.nr_samples < 3 || p.nr_samples > 8) return refuse("nr_samples must be 3 .. 8");
  if (p.k_correspondences < 1 || p.k_correspondences > kFeatK) return refuse("k_correspondences must be 1 .. 8");
  if (!(p.similarity_threshold >= 0.f && p.similarity_threshold < 1.f)) return refuse("similarity_threshold must be inside [0, 1)");
  if (!(p.inlier_fraction >= 0.f && p.inlier_fraction <= 1.f)) return refuse("inlier_fraction must be inside [0, 1]");
  if (!(p.max_corr_dist > 0.0) || !std::isfinite(p.max_corr_dist)) return refuse("max_corr_dist must be > 0 and finite");
  return OPE_OK;
}

// The draws of every iteration (host; they depend on nothing the device computes): nr_samples distinct source indices
// int(ns * next()), then nr_samples picks int(K * next()), from the LCG stream of sacia_draws.  samp / pick: H * S entries.
inline void prerej_draws(int ns, int S, int K, int H, uint64_t seed, int32_t *samp, int32_t *pick) {
  uint64_t rng = seed;
  auto next = [&rng]() {
    rng = rng * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double)(rng >> 11) * (1.0 / 9007199254740992.0);
  };
  for (int it = 0; it < H; ++it) {
    int32_t *sm = samp + (size_t)it * S;
    for (int cnt = 0; cnt < S;) {
      const int si = (int)(ns * next());
      bool fresh = true;
      for (int i = 0; i < cnt; ++i) fresh = fresh && si != sm[i];
      if (fresh) sm[cnt++] = si;
    }
    for (int i = 0; i < S; ++i) pick[(size_t)it * S + i] = (int)(K * next());
  }
}

// the accept loop over the survivors of one alignment in iteration order: a survivor is accepted iff
// (float)inliers / (float)n_src >= inlier_fraction and its error is below the lowest so far; the last accepted one, or -1
inline int64_t prerej_accept(const int32_t *inl, const double *err, size_t nsurv, int n_src, float inlier_fraction) {
  double lowest = (double)FLT_MAX;
  int64_t best = -1;
  for (size_t k = 0; k < nsurv; ++k) {
    const float frac = (float)inl[k] / (float)n_src;
    if (frac >= inlier_fraction && err[k] < lowest) { lowest = err[k]; best = (int64_t)k; }
  }
  return best;
}

__device__ __forceinline__ float edge_d2(const float4 a, const float4 b) {
  const float dx = __fsub_rn(a.x, b.x), dy = __fsub_rn(a.y, b.y), dz = __fsub_rn(a.z, b.z);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// CorrespondenceRejectorPoly with cardinality S: edge i -> (i + 1) mod S of the source polygon against the same edge of the
// target polygon, ratio of the squared lengths (the smaller over the larger) >= thr2.  A NaN ratio (0 / 0, a non-finite point) fails.
template <class Pair>
__device__ __forceinline__ bool polygon_ok(int S, float thr2, Pair pair) {
  float4 sp, tp;
  pair(0, sp, tp);
  bool ok = true;
  for (int i = 0; i < S; ++i) {
    const int j = i + 1 == S ? 0 : i + 1;   // (the first pair is fetched again for the closing edge: no per-lane array)
    float4 sn, tn;
    pair(j, sn, tn);
    const float ds = edge_d2(sp, sn), dt = edge_d2(tp, tn);
    const float ratio = ds < dt ? __fdiv_rn(ds, dt) : __fdiv_rn(dt, ds);
    ok = ok && (ratio >= thr2);
    sp = sn; tp = tn;
  }
  return ok;
}

// TransformationEstimationSVD of one hypothesis: Eigen::umeyama(src, dst, false) over its S pairs as umeyama_host runs it (means,
// centred covariance / n, rank rule, R = U S V^T, t = mean_dst - R mean_src, all fp64, cast to float at the end); the 3x3
// decomposition is svd3 of the ICP update lane.  T column-major (16), F the 3x4 [R|t] rows xform_row takes (12).
template <class Pair>
__device__ __forceinline__ void umeyama_fit(int S, Pair pair, float *__restrict__ T, float *__restrict__ F) {
  double sm[3] = {0, 0, 0}, dm[3] = {0, 0, 0};
  for (int i = 0; i < S; ++i) {
    float4 p, q;
    pair(i, p, q);
    sm[0] += p.x; sm[1] += p.y; sm[2] += p.z;
    dm[0] += q.x; dm[1] += q.y; dm[2] += q.z;
  }
  const double n = (double)S;
#pragma unroll
  for (int d = 0; d < 3; ++d) { sm[d] /= n; dm[d] /= n; }
  double sigma[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < S; ++i) {
    float4 p, q;
    pair(i, p, q);
    const double pc[3] = {p.x - sm[0], p.y - sm[1], p.z - sm[2]}, qc[3] = {q.x - dm[0], q.y - dm[1], q.z - dm[2]};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) sigma[3 * r + c] += qc[r] * pc[c];
  }
#pragma unroll
  for (int j = 0; j < 9; ++j) sigma[j] /= n;
  double U[9], sv[3], V[9];
  svd3(sigma, U, sv, V);
  double Sg[3] = {1, 1, 1};
  if (det3(sigma) < 0) Sg[2] = -1;
  int rank = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (!(fabs(sv[i]) <= fabs(sv[0]) * 1e-5)) ++rank;
  if (rank == 2) { Sg[0] = Sg[1] = 1; Sg[2] = (det3(U) * det3(V) > 0) ? 1 : -1; }
  double R[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double a = 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) a += U[3 * i + c] * Sg[c] * V[3 * j + c];
      R[3 * i + j] = a;
    }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float t = (float)(dm[i] - (R[3 * i] * sm[0] + R[3 * i + 1] * sm[1] + R[3 * i + 2] * sm[2]));
#pragma unroll
    for (int c = 0; c < 3; ++c) { const float v = (float)R[3 * i + c]; T[4 * c + i] = v; F[4 * i + c] = v; }
    T[12 + i] = t; F[4 * i + 3] = t;
    T[4 * i + 3] = 0.f;
  }
  T[15] = 1.f;
}

// The sum of one work item (a 256-thread block, one source point per lane: `in` = it is an inlier, d = its squared distance or 0):
// a butterfly over each wave's 64 lanes, then the four waves in order.  Every thread of the block calls it; thread 0 writes.
__device__ __forceinline__ void item_sum(bool in, double d, uint32_t *__restrict__ cnt_out, double *__restrict__ sum_out) {
  __shared__ double s_red[4];
  __shared__ uint32_t s_cnt[4];
  const unsigned long long b = __ballot(in);
  const double w = wave_sum(d);
  if ((threadIdx.x & 63) == 0) { s_red[threadIdx.x >> 6] = w; s_cnt[threadIdx.x >> 6] = (uint32_t)__popcll(b); }
  __syncthreads();
  if (threadIdx.x == 0) {
    *sum_out = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
    *cnt_out = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
  }
  __syncthreads();
}

// survivor k's partials in chunk order; error = sum / inliers, FLT_MAX without inliers
__device__ __forceinline__ void survivor_sum(const uint32_t *__restrict__ part_cnt, const double *__restrict__ part_sum, uint32_t k,
                                             uint32_t chunks, int32_t *__restrict__ inliers, double *__restrict__ error) {
  double sum = 0.0;
  uint32_t cnt = 0;
  for (uint32_t c = 0; c < chunks; ++c) {
    sum += part_sum[(size_t)k * chunks + c];
    cnt += part_cnt[(size_t)k * chunks + c];
  }
  inliers[k] = (int32_t)cnt;
  error[k] = cnt ? sum / (double)cnt : (double)FLT_MAX;
}

}  // namespace ope
