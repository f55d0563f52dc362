// corr_sac_math.hpp — what ope_corr_sac (corr_sac.hip) and ope_corr_sac_pose_batch (corr_sac_batch.hip) share, so that the single
// and the batched call run the same instructions: the squared descriptor distance of a match, computeSampleDistanceThreshold, the
// within-distance test and the tiled count loop, the one-block compaction of the remaining matches, the host draws and the replay of
// RandomSampleConsensus::computeModel.  DESIGN.md §4.22 has the float order of every step.
#pragma once

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <random>
#include <string>
#include <vector>

#include "feature_math.hpp"
#include "icp_update.hpp"
#include "prerejective_math.hpp"

namespace ope {

constexpr int kCsBlock = 256;            // hypotheses of one count block (one per lane)
constexpr int kCsTile = 64;              // matched pairs of one LDS tile: 2 x 64 x 16 B = 2 KB
constexpr int kCsMaxMatches = OPE_COARSE_MAX_KEYS;
constexpr int kCsPackItems = kCsMaxMatches / 1024;   // matches per lane of the one-block compaction
constexpr int kCsSumChunk = 2048;        // points the threshold kernel stages at a time (32 KB)
constexpr int kCsMaxSampleChecks = 1000; // SampleConsensusModel::max_sample_checks_
static_assert(kCsPackItems * 1024 == kCsMaxMatches, "the compaction block covers every match");

// the refusals of the parameters, the same for one call and for a batch; who: the entry point its errors name
inline int corr_sac_check_params(ope_ctx *ctx, const char *who, const ope_corr_sac_params &p) {
  const auto refuse = [&](const char *why) { return set_err(ctx, OPE_EINVAL, std::string(who) + why); };
  if (p.max_iterations < 1 || p.max_iterations > kPrMaxIterations) return refuse("max_iterations must be 1 .. 2^20");
  if (!(p.inlier_threshold > 0.0) || !std::isfinite(p.inlier_threshold)) return refuse("inlier_threshold must be > 0 and finite");
  if (!(p.probability > 0.0 && p.probability < 1.0)) return refuse("probability must be inside (0, 1)");
  return OPE_OK;
}

// the squared distance of query row q to target row t (t < 0: no match, infinity): feature_knn_block's sequential float sum
__device__ __forceinline__ float cs_row_dist(const float *__restrict__ tgt_feat, const float *__restrict__ q, int32_t t) {
  float d = INFINITY;
  if (t >= 0) {
    const float *f = tgt_feat + (size_t)t * 33;
    d = 0.f;
    for (int c = 0; c < 33; ++c) { const float u = q[c] - f[c]; d += u * u; }
  }
  return d;
}

// computeSampleDistanceThreshold over the n >= 1 matched source points ps (one block of kCsBlock lanes): the nine running sums of
// computeMeanAndCovarianceMatrix in match order, lane j the j-th (xx xy xz yy yz zz x y z; the last three multiply by 1, which is
// exact), then pcl::eigen33 (mat, evals): the roots of the matrix over its largest entry, times it; t = ((sqrt l0 + sqrt l1) +
// sqrt l2) in float, over 3.0 and squared in double.
__device__ __forceinline__ void cs_thresh_block(const float4 *__restrict__ ps, uint32_t n, double *__restrict__ out_thr) {
  __shared__ float4 s_p[kCsSumChunk];
  __shared__ float s_acc[9];
  const int j = threadIdx.x;
  const int ia = j < 3 ? 0 : j < 5 ? 1 : j < 6 ? 2 : j - 6;          // first factor: x x x y y z | x y z
  const int ib = j < 3 ? j : j < 5 ? j - 2 : j < 6 ? 2 : 3;           // second factor: x y z y z z | 1 1 1
  float acc = 0.f;
  for (uint32_t base = 0; base < n; base += kCsSumChunk) {
    const uint32_t m = min((uint32_t)kCsSumChunk, n - base);
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < m; k += kCsBlock) {
      const float4 p = ps[base + k];
      s_p[k] = make_float4(p.x, p.y, p.z, 1.f);
    }
    __syncthreads();
    if (j < 9)
      for (uint32_t k = 0; k < m; ++k) {
        const float *p = reinterpret_cast<const float *>(&s_p[k]);
        acc = __fadd_rn(acc, __fmul_rn(p[ia], p[ib]));
      }
  }
  if (j < 9) s_acc[j] = acc;
  __syncthreads();
  if (j != 0) return;
  float accu[9];
  const float fc = (float)n;
#pragma unroll
  for (int a = 0; a < 9; ++a) accu[a] = __fdiv_rn(s_acc[a], fc);
  float cov[9];
  cov[0] = __fsub_rn(accu[0], __fmul_rn(accu[6], accu[6]));
  cov[1] = __fsub_rn(accu[1], __fmul_rn(accu[6], accu[7]));
  cov[2] = __fsub_rn(accu[2], __fmul_rn(accu[6], accu[8]));
  cov[4] = __fsub_rn(accu[3], __fmul_rn(accu[7], accu[7]));
  cov[5] = __fsub_rn(accu[4], __fmul_rn(accu[7], accu[8]));
  cov[8] = __fsub_rn(accu[5], __fmul_rn(accu[8], accu[8]));
  cov[3] = cov[1]; cov[6] = cov[2]; cov[7] = cov[5];
  float scale = 0.f;
#pragma unroll
  for (int i = 0; i < 9; ++i) scale = fmaxf(scale, fabsf(cov[i]));
  if (scale <= 1.17549435e-38f) scale = 1.0f;
  float sm[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) sm[i] = __fdiv_rn(cov[i], scale);
  float roots[3];
  compute_roots(sm, roots);
  const float r0 = __fsqrt_rn(__fmul_rn(roots[0], scale)), r1 = __fsqrt_rn(__fmul_rn(roots[1], scale)), r2 = __fsqrt_rn(__fmul_rn(roots[2], scale));
  const double t = (double)__fadd_rn(__fadd_rn(r0, r1), r2) / 3.0;
  out_thr[0] = t * t;
}

// a match is within the distance iff |T s - t|^2 < thr2: the point moved by xform_row, the squared norm (dx dx + dy dy) + dz dz in
// float, widened
__device__ __forceinline__ bool cs_within(const float F[12], const float4 s, const float4 t, double thr2) {
  const float dx = __fsub_rn(xform_row(F + 0, s.x, s.y, s.z), t.x);
  const float dy = __fsub_rn(xform_row(F + 4, s.x, s.y, s.z), t.y);
  const float dz = __fsub_rn(xform_row(F + 8, s.x, s.y, s.z), t.z);
  const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
  return (double)d2 < thr2;
}

// countWithinDistance of one hypothesis per lane (a block of kCsBlock lanes, F = the lane's 3x4 rows) over the tiles first_tile,
// first_tile + tile_stride, ... of the n matched pairs.  A tile is staged once per block (a lane of the first wave loads one pair)
// and read by every lane at the same address: a broadcast, no bank conflict.  Every lane of the block calls it.
__device__ __forceinline__ uint32_t cs_count_tiles(const float4 *__restrict__ ps, const float4 *__restrict__ pt, uint32_t n, const float F[12],
                                                   double thr2, uint32_t first_tile, uint32_t tile_stride) {
  __shared__ float4 s_s[kCsTile], s_t[kCsTile];
  uint32_t cnt = 0;
  for (uint32_t base = first_tile * kCsTile; base < n; base += tile_stride * kCsTile) {
    const uint32_t m = min((uint32_t)kCsTile, n - base);
    __syncthreads();
    if (threadIdx.x < m) { s_s[threadIdx.x] = ps[base + threadIdx.x]; s_t[threadIdx.x] = pt[base + threadIdx.x]; }
    __syncthreads();
#pragma unroll 4
    for (uint32_t k = 0; k < m; ++k) cnt += cs_within(F, s_s[k], s_t[k], thr2) ? 1u : 0u;
  }
  return cnt;
}

// The exclusive prefix of `mine` over a block of 1024 lanes (within the wave by shuffles, the sixteen waves through LDS) and the
// block's total.  Every lane calls it; it ends with a barrier, so a block may call it again.
__device__ __forceinline__ uint32_t cs_block_prefix(uint32_t mine, uint32_t &total) {
  __shared__ uint32_t s_wave[16];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t inc = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t v = __shfl_up(inc, off, 64);
    if (lane >= (uint32_t)off) inc += v;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  uint32_t before = 0;
  total = 0;
  for (uint32_t w = 0; w < 16; ++w) {
    if (w < wave) before += s_wave[w];
    total += s_wave[w];
  }
  __syncthreads();
  return before + inc - mine;
}

// selectWithinDistance of the hypothesis F (all != 0: every match), compacted in match order by one block of 1024 lanes: lane l owns
// the matches [kCsPackItems l, kCsPackItems l + kCsPackItems).  Positions, and the pairs packed as xyz for the pairs-sum kernel.
__device__ __forceinline__ void cs_pack_block(const float4 *__restrict__ ps, const float4 *__restrict__ pt, uint32_t n, const float F[12],
                                              double thr2, int all, int32_t *__restrict__ pos, float *__restrict__ sx, float *__restrict__ tx,
                                              uint32_t *__restrict__ d_cnt) {
  bool in[kCsPackItems];
  uint32_t mine = 0;
#pragma unroll
  for (int a = 0; a < kCsPackItems; ++a) {
    const uint32_t i = threadIdx.x * kCsPackItems + a;
    in[a] = i < n && (all || cs_within(F, ps[i], pt[i], thr2));
    mine += in[a] ? 1u : 0u;
  }
  uint32_t total;
  uint32_t slot = cs_block_prefix(mine, total);
#pragma unroll
  for (int a = 0; a < kCsPackItems; ++a) {
    if (!in[a]) continue;
    const uint32_t i = threadIdx.x * kCsPackItems + a;
    const float4 s = ps[i], t = pt[i];
    pos[slot] = (int32_t)i;
    sx[3 * slot] = s.x; sx[3 * slot + 1] = s.y; sx[3 * slot + 2] = s.z;
    tx[3 * slot] = t.x; tx[3 * slot + 1] = t.y; tx[3 * slot + 2] = t.z;
    ++slot;
  }
  if (threadIdx.x == 0) *d_cnt = total;
}

inline float edge_d2_host(const float4 &a, const float4 &b) {
  const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
  return (dx * dx + dy * dy) + dz * dz;   // (the library is compiled without contraction)
}

// getSamples for the H consecutive iterations RANSAC can run: a persistent shuffled_indices_ over all matches, drawIndexSample's three
// swaps with rnd() = engine() >> 1, up to 1000 redraws while isSampleGood fails (an edge of the source triangle not above the
// threshold).  The list ends where getSamples would hand back an empty selection.
inline void cs_draw(const float4 *ps, int n, double thr, uint32_t seed, size_t H, std::vector<int32_t> &samp) {
  std::mt19937 eng(seed);
  std::vector<int32_t> shuf((size_t)n);
  for (int i = 0; i < n; ++i) shuf[(size_t)i] = i;
  samp.clear();
  samp.reserve(3 * H);
  for (size_t h = 0; h < H; ++h) {
    bool good = false;
    for (int check = 0; check < kCsMaxSampleChecks && !good; ++check) {
      for (int i = 0; i < 3; ++i) std::swap(shuf[(size_t)i], shuf[(size_t)i + (size_t)((eng() >> 1) % (uint32_t)(n - i))]);
      const float4 &p0 = ps[shuf[0]], &p1 = ps[shuf[1]], &p2 = ps[shuf[2]];
      good = (double)edge_d2_host(p1, p0) > thr && (double)edge_d2_host(p2, p0) > thr && (double)edge_d2_host(p2, p1) > thr;
    }
    if (!good) return;
    samp.insert(samp.end(), shuf.begin(), shuf.begin() + 3);
  }
}

// RandomSampleConsensus::computeModel, replayed over the counts of the H hypotheses drawn for n matches: the draws did not depend
// on the counts, so hypothesis `it` is the one iteration `it` would have drawn.  Returns iterations_; *best = the winner (-1
// without one), *best_cnt its count.
inline int cs_replay(const uint32_t *cnts, uint32_t H, size_t n, int max_iterations, double probability, int *best, long long *best_cnt) {
  *best = -1;
  *best_cnt = -(long long)INT_MAX;
  double k = 1.0;
  int it = 0;
  const double log_probability = std::log(1.0 - probability);
  while ((double)it < k) {
    if ((uint32_t)it >= H) break;   // an empty selection
    const long long c = (long long)cnts[(size_t)it];
    if (c > *best_cnt) {
      *best_cnt = c;
      *best = it;
      const double w = (double)*best_cnt / (double)n;
      double p_no_outliers = 1.0 - std::pow(w, 3.0);
      p_no_outliers = std::max(DBL_EPSILON, p_no_outliers);
      p_no_outliers = std::min(1.0 - DBL_EPSILON, p_no_outliers);
      k = log_probability / std::log(p_no_outliers);
    }
    ++it;
    if (it > max_iterations) break;
  }
  return it;
}

}  // namespace ope
