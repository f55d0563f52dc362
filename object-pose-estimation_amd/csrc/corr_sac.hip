// corr_sac.hip — the correspondence pipeline the reference keeps commented out in estimateCoarsePose
// (BuildModel/src/poseestimator.cpp:43-60, :111-113) on the device (gfx950, wave64): a 1-NN match of every source FPFH row in the
// target's rows (pcl::registration::CorrespondenceEstimation), pcl::registration::CorrespondenceRejectorSampleConsensus over the
// matches (RandomSampleConsensus on SampleConsensusModelRegistration) and TransformationEstimationSVD over the matches that remain.
// DESIGN.md §4.22 has the float order of every step; tests/corr_sac_ref.py is the specification.
//
// ope_feature_correspondences: one block per source row over feature_knn_block with k = 1; it also writes the distance.
//
// ope_corr_sac:
//   1. two launches restore the ORIGINAL order of both clouds, one gathers the matched pairs in match order;
//   2. nine lanes of one block add computeMeanAndCovarianceMatrix's nine running float sums in match order (a sequential float sum
//      cannot be split), one lane takes the eigenvalues (compute_roots, the device's eigen33) and sample_dist_thresh; the matched
//      source points and the threshold come down in one copy (first synchronisation);
//   3. the host draws every sample RANSAC can reach (std::mt19937, drawIndexSample's three swaps, isSampleGood with up to 1000
//      redraws) and uploads them in one copy;
//   4. one lane per hypothesis fits Umeyama over its three pairs (umeyama_fit);
//   5. the hot kernel scores every hypothesis against every match: the pairs go through LDS in tiles, a lane keeps its hypothesis's
//      twelve floats in registers and walks the tile with broadcast reads; the matches are split over work items when the
//      hypotheses alone do not fill the device, and the partial counts meet in integer atomics;
//   6. transforms and counts come back (second synchronisation); the host replays RandomSampleConsensus::computeModel;
//   7. one block marks and compacts the winner's inliers (all matches without a model), the pairs-sum kernel and the Umeyama lane of
//      ope_rigid_transform_svd fit them; positions and pose come back (third synchronisation).
// No launch count and no synchronisation count depends on the hypotheses, the matches, the iteration RANSAC stops at or the inliers.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "coarse_stages.hpp"
#include "corr_sac_math.hpp"
#include "stage_host.hpp"

namespace ope {

namespace {

static_assert(12ull * ((size_t)kPrMaxIterations + 1) <= kStageChunk, "the samples go up in one staged copy");

// the match of one source row per block: the nearest target row (feature_knn_block, k = 1) and its squared distance, the same
// sequential float sum
__global__ __launch_bounds__(256) void cs_match_kernel(const float *__restrict__ tgt_feat, int nt, const float *__restrict__ src_feat,
                                                        int32_t *__restrict__ out_idx, float *__restrict__ out_d) {
  const float *q = src_feat + (size_t)blockIdx.x * 33;
  feature_knn_block(tgt_feat, nt, q, 1, out_idx + blockIdx.x);
  if (threadIdx.x == 0) out_d[blockIdx.x] = cs_row_dist(tgt_feat, q, out_idx[blockIdx.x]);
}

// 1a. original order
__global__ __launch_bounds__(kCsBlock) void cs_orig_kernel(CloudView c, float4 *__restrict__ pts_o) {
  const uint32_t p = blockIdx.x * kCsBlock + threadIdx.x;
  if (p >= c.n) return;
  const float4 q = c.xyzw[p];
  const uint32_t o = (uint32_t)__float_as_int(q.w);
  if (o < c.n) pts_o[o] = q;
}

// 1b. the pairs in match order
__global__ __launch_bounds__(kCsBlock) void cs_gather_kernel(const float4 *__restrict__ src_o, const float4 *__restrict__ tgt_o,
                                                             const int32_t *__restrict__ si, const int32_t *__restrict__ ti, uint32_t n,
                                                             float4 *__restrict__ ps, float4 *__restrict__ pt) {
  const uint32_t i = blockIdx.x * kCsBlock + threadIdx.x;
  if (i >= n) return;
  const float4 s = src_o[si[i]], t = tgt_o[ti[i]];
  ps[i] = make_float4(s.x, s.y, s.z, 0.f);
  pt[i] = make_float4(t.x, t.y, t.z, 0.f);
}

// 2. computeSampleDistanceThreshold (cs_thresh_block)
__global__ __launch_bounds__(kCsBlock) void cs_thresh_kernel(const float4 *__restrict__ ps, uint32_t n, double *__restrict__ out_thr) {
  cs_thresh_block(ps, n, out_thr);
}

// 4. computeModelCoefficients: one lane per hypothesis, Umeyama without scaling over its three pairs
__global__ __launch_bounds__(64) void cs_fit_kernel(const float4 *__restrict__ ps, const float4 *__restrict__ pt, const int32_t *__restrict__ samp,
                                                    uint32_t H, float *__restrict__ T_out, float *__restrict__ rows_out) {
  const uint32_t h = blockIdx.x * 64 + threadIdx.x;
  if (h >= H) return;
  const int32_t *sa = samp + 3 * (size_t)h;
  umeyama_fit(3, [&](int i, float4 &p, float4 &q) { p = ps[sa[i]]; q = pt[sa[i]]; }, T_out + 16 * (size_t)h, rows_out + 12 * (size_t)h);
}

// 5. countWithinDistance of every hypothesis: block (x, y) = hypotheses [256 x, 256 x + 256) against the tiles y, y + gridDim.y, ...
// of the matches (cs_count_tiles).  Counts are integers: the atomics' order does not show.
__global__ __launch_bounds__(kCsBlock) void cs_count_kernel(const float4 *__restrict__ ps, const float4 *__restrict__ pt, uint32_t n,
                                                            const float *__restrict__ rows, uint32_t H, double thr2,
                                                            uint32_t *__restrict__ counts) {
  const uint32_t h = blockIdx.x * kCsBlock + threadIdx.x;
  const bool live = h < H;
  float F[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) F[i] = live ? rows[12 * (size_t)h + i] : 0.f;
  const uint32_t cnt = cs_count_tiles(ps, pt, n, F, thr2, blockIdx.y, gridDim.y);
  if (live && cnt) atomicAdd(counts + h, cnt);
}

// 7. selectWithinDistance of the winner (all != 0: every match), compacted in match order by one block of 1024 lanes (cs_pack_block)
__global__ __launch_bounds__(1024) void cs_pack_kernel(const float4 *__restrict__ ps, const float4 *__restrict__ pt, uint32_t n,
                                                        const float *__restrict__ F_in, double thr2, int all, int32_t *__restrict__ pos,
                                                        float *__restrict__ sx, float *__restrict__ tx, uint32_t *__restrict__ d_cnt) {
  float F[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) F[i] = F_in[i];
  cs_pack_block(ps, pt, n, F, thr2, all, pos, sx, tx, d_cnt);
}

}  // namespace
}  // namespace ope

using namespace ope;

extern "C" {

int ope_feature_correspondences(ope_ctx *ctx, const float *src_feat33, size_t n_src, const float *tgt_feat33, size_t n_tgt, int32_t *out_src_idx,
                                int32_t *out_tgt_idx, float *out_dist, size_t *n_out) {
  static const char *who = "ope_feature_correspondences: ";
  if (!ctx) return OPE_EINVAL;
  if (n_out) *n_out = 0;
  if (!n_out || !out_src_idx || !out_tgt_idx || (n_src && !src_feat33) || (n_tgt && !tgt_feat33))
    return set_err(ctx, OPE_EINVAL, std::string(who) + "bad argument");
  if (n_src > (size_t)0x7fffffff || n_tgt > (size_t)0x7fffffff) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than 2^31 - 1 rows");
  if (n_src == 0 || n_tgt == 0) return OPE_OK;
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  TraceRange r(ctx, "feature_correspondences");
  const hipStream_t st = ctx->stream;
  CallTmp tmp{st, {}};
  hipError_t e = hipSuccess;
  const size_t sb = 132 * n_src, tb = 132 * n_tgt;
  auto *d_sf = (float *)tmp.get(sb, e);
  auto *d_tf = (float *)tmp.get(tb, e);
  auto *d_back = (unsigned char *)tmp.get(8 * n_src, e);
  if (e == hipSuccess) e = h2d_copy(st, d_sf, src_feat33, sb);
  if (e == hipSuccess) e = h2d_copy(st, d_tf, tgt_feat33, tb);
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  STAGE_LAUNCH_TIMED(ctx, cs_match_kernel, "cs_match_kernel", 132.0 * ((double)n_src * (double)n_tgt + (double)n_src), dim3((unsigned)n_src), dim3(256), 0, st,
                     (const float *)d_tf, (int)n_tgt, (const float *)d_sf, (int32_t *)d_back, (float *)(d_back + 4 * n_src));
  std::vector<unsigned char> back(8 * n_src);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(back.data(), d_back, back.size(), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  const auto *idx = (const int32_t *)back.data();
  const auto *dist = (const float *)(back.data() + 4 * n_src);
  size_t m = 0;
  for (size_t i = 0; i < n_src; ++i) {
    if (idx[i] < 0 || (size_t)idx[i] >= n_tgt) continue;   // no finite distance: no match
    out_src_idx[m] = (int32_t)i;
    out_tgt_idx[m] = idx[i];
    if (out_dist) out_dist[m] = dist[i];
    ++m;
  }
  *n_out = m;
  return OPE_OK;
}

void ope_corr_sac_default_params(ope_corr_sac_params *p) {
  if (!p) return;
  p->inlier_threshold = 0.05;   /* CorrespondenceRejectorSampleConsensus's own default */
  p->max_iterations = 1000;
  p->probability = 0.99;        /* SampleConsensus::probability_ */
  p->seed = 12345;              /* SampleConsensusModel's engine without a random seed */
}

int ope_corr_sac(ope_ctx *ctx, const ope_cloud *src, const ope_cloud *tgt, const int32_t *src_idx, const int32_t *tgt_idx, size_t n,
                 const ope_corr_sac_params *params, const int32_t *forced_samples, size_t n_forced, ope_corr_sac_result *out,
                 int32_t *out_inlier_pos) {
  static const char *who = "ope_corr_sac: ";
  if (!ctx) return OPE_EINVAL;
  if (out) {
    std::memcpy(out->T_best, kIdentity4, sizeof kIdentity4);
    std::memcpy(out->T_svd, kIdentity4, sizeof kIdentity4);
    out->inliers = 0;
    out->best = -1;
    out->iterations = 0;
    out->found = 0;
  }
  if (!src || !tgt || !out || (n && (!src_idx || !tgt_idx)) || (n_forced && !forced_samples))
    return set_err(ctx, OPE_EINVAL, std::string(who) + "bad argument");
  ope_corr_sac_params p;
  ope_corr_sac_default_params(&p);
  if (params) p = *params;
  if (const int rc = corr_sac_check_params(ctx, who, p)) return rc;
  if (n > (size_t)kCsMaxMatches) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than OPE_COARSE_MAX_KEYS matches");
  if (n_forced > (size_t)kPrMaxIterations + 1) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than 2^20 + 1 forced samples");
  if (src->n > (size_t)0x7fffffff || tgt->n > (size_t)0x7fffffff) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than 2^31 - 1 points");
  if (const int rc = refuse_communicator(ctx, who)) return rc;
  for (size_t i = 0; i < n; ++i)
    if (src_idx[i] < 0 || (size_t)src_idx[i] >= src->n || tgt_idx[i] < 0 || (size_t)tgt_idx[i] >= tgt->n)
      return set_err(ctx, OPE_EINVAL, std::string(who) + "match index out of range");
  {
    std::vector<int32_t> seen(src_idx, src_idx + n);
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
      return set_err(ctx, OPE_EINVAL, std::string(who) + "a source index occurs in two matches");
  }
  for (int side = 0; side < 2; ++side) {   // a cloud with non-finite points: its host mirror says which
    const ope_cloud *c = side ? tgt : src;
    const int32_t *ix = side ? tgt_idx : src_idx;
    if (c->n_valid == c->n || n == 0) continue;
    const int rch = c->ensure_host();
    if (rch != OPE_OK) return rch;
    for (size_t i = 0; i < n; ++i) {
      const float *q = &c->h_xyz[3 * (size_t)ix[i]];
      if (!(std::isfinite(q[0]) && std::isfinite(q[1]) && std::isfinite(q[2])))
        return set_err(ctx, OPE_EINVAL, std::string(who) + "a match on a non-finite point");
    }
  }
  for (size_t j = 0; j < 3 * n_forced; ++j)
    if (forced_samples[j] < 0 || (size_t)forced_samples[j] >= n) return set_err(ctx, OPE_EINVAL, std::string(who) + "sample index out of range");
  ope_corr_sac_stats &St = ctx->corr_sac_stats;
  St = ope_corr_sac_stats{};
  ctx->corr_sac_samples.clear(); ctx->corr_sac_T.clear(); ctx->corr_sac_counts.clear();
  if (n == 0) return OPE_OK;   // nothing to reject and nothing to fit: no model, the identity
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  TraceRange r_cs(ctx, "corr_sac");
  const hipStream_t st = ctx->stream;
  CallTmp tmp{st, {}};
  hipError_t e = hipSuccess;
  const uint32_t nn = (uint32_t)n;
  const size_t Hmax = n_forced ? n_forced : (size_t)p.max_iterations + 1;

  // ---- 1, 2. the pairs in match order, the threshold
  auto *src_o = (float4 *)tmp.get(16 * std::max<size_t>(src->n, 1), e);
  auto *tgt_o = (float4 *)tmp.get(16 * std::max<size_t>(tgt->n, 1), e);
  auto *d_idx = (int32_t *)tmp.get(8 * n, e);
  auto *d_down = (unsigned char *)tmp.get(16 * n + 16, e);   // [matched source points | threshold]
  auto *d_pt = (float4 *)tmp.get(16 * n, e);
  auto *d_samp = (int32_t *)tmp.get(12 * Hmax, e);
  auto *d_back = (unsigned char *)tmp.get(68 * Hmax, e);     // [T | counts]
  auto *d_rows = (float *)tmp.get(48 * Hmax, e);
  auto *d_pos = (int32_t *)tmp.get(4 * n + 128, e);           // [positions | count | T_svd]
  auto *d_sx = (float *)tmp.get(12 * n, e);
  auto *d_tx = (float *)tmp.get(12 * n, e);
  auto *d_wrows = (float *)tmp.get(48, e);
  const int svd_blocks_max = (int)std::min<size_t>((n + 255) / 256, 512);
  auto *d_part = (double *)tmp.get(sizeof(double) * kNumSums * (size_t)svd_blocks_max, e);
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  auto *d_ps = (float4 *)d_down;
  auto *d_thr = (double *)(d_down + 16 * n);
  {
    std::vector<int32_t> both(2 * n);
    std::memcpy(both.data(), src_idx, 4 * n);
    std::memcpy(both.data() + n, tgt_idx, 4 * n);
    e = upload_staged(st, d_idx, both.data(), 8 * n, &St.launches, &St.host_syncs);   // (at most 32 KB: one copy, no synchronisation)
  }
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  STAGE_LAUNCH(ctx, St.launches, cs_orig_kernel, 32.0 * src->n, dim3(grid_of(src->n, kCsBlock)), dim3(kCsBlock), 0, st, src->view(), src_o);
  STAGE_LAUNCH(ctx, St.launches, cs_orig_kernel, 32.0 * tgt->n, dim3(grid_of(tgt->n, kCsBlock)), dim3(kCsBlock), 0, st, tgt->view(), tgt_o);
  STAGE_LAUNCH(ctx, St.launches, cs_gather_kernel, 72.0 * n, dim3(grid_of(n, kCsBlock)), dim3(kCsBlock), 0, st, (const float4 *)src_o, (const float4 *)tgt_o,
               (const int32_t *)d_idx, (const int32_t *)(d_idx + n), nn, d_ps, d_pt);
  STAGE_LAUNCH(ctx, St.launches, cs_thresh_kernel, 16.0 * n, dim3(1), dim3(kCsBlock), 0, st, (const float4 *)d_ps, nn, d_thr);
  std::vector<unsigned char> down(16 * n + 16);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(down.data(), d_down, down.size(), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  ++St.host_syncs;
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + "(pairs) " + hipGetErrorString(e));
  double thr = 0.0;
  std::memcpy(&thr, down.data() + 16 * n, 8);
  St.sample_dist_thresh = thr;

  // ---- 3. the draws (fewer than 3 matches: none, and no model)
  std::vector<int32_t> samp;
  if (n >= 3) {
    if (n_forced) samp.assign(forced_samples, forced_samples + 3 * n_forced);
    else cs_draw((const float4 *)down.data(), (int)n, thr, (uint32_t)(p.seed & 0xffffffffull), Hmax, samp);
  }
  const uint32_t H = (uint32_t)(samp.size() / 3);
  St.hypotheses = H;
  {
    std::vector<int32_t> up(samp);
    up.resize(std::max<size_t>(up.size(), 3), 0);   // (one copy whether or not anything was drawn)
    e = upload_staged(st, d_samp, up.data(), 4 * up.size(), &St.launches, &St.host_syncs);   // (at most 12 MB: one copy, no synchronisation)
  }
  if (e == hipSuccess) e = hipMemsetAsync(d_back + 64 * Hmax, 0, 4 * Hmax, st);
  ++St.launches;
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));

  // ---- 4, 5. fits and counts
  const double thr2 = p.inlier_threshold * p.inlier_threshold;
  auto *d_T = (float *)d_back;
  auto *d_cnt = (uint32_t *)(d_back + 64 * Hmax);
  STAGE_LAUNCH(ctx, St.launches, cs_fit_kernel, 208.0 * H, dim3(grid_of(H, 64)), dim3(64), 0, st, (const float4 *)d_ps, (const float4 *)d_pt,
               (const int32_t *)d_samp, H, d_T, d_rows);
  const unsigned hb = grid_of(H, kCsBlock), tiles = grid_of(n, kCsTile);
  const unsigned split = std::min(tiles, std::max(1u, (2u * (unsigned)ctx->n_cu + hb - 1) / hb));
  STAGE_LAUNCH(ctx, St.launches, cs_count_kernel, 32.0 * n * hb + 52.0 * H, dim3(hb, split), dim3(kCsBlock), 0, st, (const float4 *)d_ps, (const float4 *)d_pt,
               nn, (const float *)d_rows, H, thr2, d_cnt);
  std::vector<float> Ts(16 * std::max<size_t>(H, 1));
  std::vector<uint32_t> cnts(std::max<size_t>(H, 1));
  e = hipGetLastError();
  if (e == hipSuccess && H) e = hipMemcpyAsync(Ts.data(), d_T, 64 * (size_t)H, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && H) e = hipMemcpyAsync(cnts.data(), d_cnt, 4 * (size_t)H, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  ++St.host_syncs;
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + "(counts) " + hipGetErrorString(e));
  ctx->corr_sac_samples = samp;
  ctx->corr_sac_T.assign(Ts.begin(), Ts.begin() + 16 * (size_t)H);
  ctx->corr_sac_counts.assign(cnts.begin(), cnts.begin() + H);

  // ---- 6. RandomSampleConsensus::computeModel, replayed: the draws did not depend on the counts, so hypothesis `it` is the one
  // iteration `it` would have drawn
  int best = -1;
  long long best_cnt = 0;
  const int it = cs_replay(cnts.data(), H, n, p.max_iterations, p.probability, &best, &best_cnt);
  St.iterations = it;
  out->iterations = it;
  out->best = best;
  out->found = best >= 0 ? 1 : 0;
  if (best >= 0) std::memcpy(out->T_best, &Ts[16 * (size_t)best], 64);

  // ---- 7. the remaining matches and their pose (without a model: every match)
  const uint32_t n_rem = best >= 0 ? (uint32_t)best_cnt : nn;
  float wrows[12];
  colmajor_to_rows12(out->T_best, wrows);
  e = h2d_copy(st, d_wrows, wrows, 48);
  ++St.launches;
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  auto *d_pcnt = (uint32_t *)((unsigned char *)d_pos + 4 * n);
  auto *d_Tsvd = (float *)((unsigned char *)d_pos + 4 * n + 64);
  STAGE_LAUNCH(ctx, St.launches, cs_pack_kernel, 92.0 * n, dim3(1), dim3(1024), 0, st, (const float4 *)d_ps, (const float4 *)d_pt, nn, (const float *)d_wrows,
               thr2, best >= 0 ? 0 : 1, d_pos, d_sx, d_tx, d_pcnt);
  {
    // (the two launches of ope_rigid_transform_svd, with its grid: the same bits for the same pairs)
    KernelTimer kt(ctx, "cs_pairs_svd", 24.0 * n_rem);
    const int nblocks = (int)std::max<size_t>(std::min<size_t>(((size_t)n_rem + 255) / 256, 512), 1);
    launch_pairs_svd(st, d_sx, d_tx, n_rem, d_part, nblocks, d_Tsvd);
    St.launches += 2;
  }
  std::vector<unsigned char> fin(4 * n + 128);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(fin.data(), d_pos, fin.size(), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  ++St.host_syncs;
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + "(inliers) " + hipGetErrorString(e));
  uint32_t packed = 0;
  std::memcpy(&packed, fin.data() + 4 * n, 4);
  if (packed != n_rem) return set_err(ctx, OPE_EHIP, std::string(who) + "the winner's inlier list and its count disagree");
  out->inliers = (int32_t)n_rem;
  if (out_inlier_pos && n_rem) std::memcpy(out_inlier_pos, fin.data(), 4 * (size_t)n_rem);
  if (n_rem) std::memcpy(out->T_svd, fin.data() + 4 * n + 64, 64);
  return OPE_OK;
}

int ope_corr_sac_last_stats(const ope_ctx *ctx, ope_corr_sac_stats *out) {
  if (!ctx || !out) return OPE_EINVAL;
  *out = ctx->corr_sac_stats;
  return OPE_OK;
}

int ope_corr_sac_last_hypotheses(const ope_ctx *ctx, int32_t *samples, float *T, int32_t *counts, size_t cap, size_t *n_out) {
  if (!ctx || !n_out) return OPE_EINVAL;
  const size_t made = ctx->corr_sac_counts.size(), w = std::min(made, cap);
  if (samples && w) std::memcpy(samples, ctx->corr_sac_samples.data(), 12 * w);
  if (T && w) std::memcpy(T, ctx->corr_sac_T.data(), 64 * w);
  if (counts && w) std::memcpy(counts, ctx->corr_sac_counts.data(), 4 * w);
  *n_out = made;
  return OPE_OK;
}

}  // extern "C"
