// prerejective.hip — pcl::SampleConsensusPrerejective on the device (gfx950, wave64): the coarse alignment the reference's author
// left commented out in BuildModel/src/poseestimator.cpp:90-108 (50 000 iterations of 3 samples, too slow on one CPU thread).
// DESIGN.md §4.20 has the float order of every step.
//
// ope_prerejective:
//   1. two launches restore the ORIGINAL order of both clouds (clouds are stored along the Morton curve, w = original index);
//   2. the host draws every iteration's samples and picks (the LCG of sacia_draws; the draws depend on nothing the device
//      computes); one launch finds the k nearest target descriptors of every distinct sampled source point (feature_knn_block)
//      and the picks become target indices (first synchronisation);
//   3. one lane per iteration runs CorrespondenceRejectorPoly's edge tests and writes a flag; a rocPRIM select keeps the survivors
//      in iteration order; their number comes back (second synchronisation);
//   4. one lane per survivor fits Umeyama without scaling in fp64 (the operations of umeyama_host, svd3 for the decomposition);
//   5. one work item per (survivor, 256 source points) takes the exact 1-NN distance of every moved point and writes an inlier count
//      and an fp64 partial sum; one lane per survivor adds its partials in chunk order: the order of a sum depends on the source
//      cloud alone, never on the launch;
//   6. transforms, counts and errors come back (third synchronisation) and the host replays the accept loop in iteration order;
//   7. on request one more pass writes the winner's inliers (flags by original index, a select; fourth synchronisation).
// No launch count and no synchronisation count depends on the iterations, the survivors or the points.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "coarse_stages.hpp"
#include "feature_math.hpp"
#include "icp_update.hpp"
#include "prerejective_math.hpp"
#include "stage_host.hpp"

namespace ope {
namespace {

// 1. original order
__global__ __launch_bounds__(kPrBlock) void prerej_orig_kernel(CloudView c, float4 *__restrict__ pts_o) {
  const uint32_t p = blockIdx.x * kPrBlock + threadIdx.x;
  if (p >= c.n) return;
  const float4 q = c.xyzw[p];
  const uint32_t o = (uint32_t)__float_as_int(q.w);
  if (o < c.n) pts_o[o] = q;
}

// 2. findSimilarFeatures of one distinct sampled source point per block
__global__ __launch_bounds__(256) void prerej_feature_knn_kernel(const float *__restrict__ tgt_feat, int nt, const float *__restrict__ q_feat, int k,
                                                                  int32_t *__restrict__ out_idx) {
  feature_knn_block(tgt_feat, nt, q_feat + (size_t)blockIdx.x * 33, k, out_idx + (size_t)blockIdx.x * k);
}

// 3. CorrespondenceRejectorPoly with cardinality S: edge i -> (i + 1) mod S of the source polygon against the same edge of the
// target polygon, ratio of the squared lengths (the smaller over the larger) >= thr2.  A NaN ratio (0 / 0, a non-finite point) fails.
__global__ __launch_bounds__(kPrBlock) void prerej_polygon_kernel(const float4 *__restrict__ src_o, const float4 *__restrict__ tgt_o,
                                                                  const int32_t *__restrict__ samp, const int32_t *__restrict__ corr, uint32_t H,
                                                                  int S, float thr2, uint8_t *__restrict__ flags) {
  const uint32_t it = blockIdx.x * kPrBlock + threadIdx.x;
  if (it >= H) return;
  const int32_t *sa = samp + (size_t)it * S, *co = corr + (size_t)it * S;
  const bool ok = polygon_ok(S, thr2, [&](int i, float4 &s, float4 &t) { s = src_o[sa[i]]; t = tgt_o[co[i]]; });
  flags[it] = ok ? 1 : 0;
}

// 4. TransformationEstimationSVD of one survivor: Eigen::umeyama(src, dst, false) over its S pairs as umeyama_host runs it (means,
// centred covariance / n, rank rule, R = U S V^T, t = mean_dst - R mean_src, all fp64, cast to float at the end); the 3x3
// decomposition is svd3 of the ICP update lane.  T column-major, rows = the 3x4 [R|t] rows xform_row takes.
__global__ __launch_bounds__(64) void prerej_fit_kernel(const float4 *__restrict__ src_o, const float4 *__restrict__ tgt_o,
                                                        const int32_t *__restrict__ samp, const int32_t *__restrict__ corr, int S,
                                                        const int32_t *__restrict__ surv, const uint32_t *__restrict__ d_nsurv,
                                                        float *__restrict__ T_out, float *__restrict__ rows_out) {
  const uint32_t k = blockIdx.x * 64 + threadIdx.x;
  if (k >= *d_nsurv) return;
  const int32_t it = surv[k];
  const int32_t *sa = samp + (size_t)it * S, *co = corr + (size_t)it * S;
  umeyama_fit(S, [&](int i, float4 &p, float4 &q) { p = src_o[sa[i]]; q = tgt_o[co[i]]; }, T_out + 16 * (size_t)k, rows_out + 12 * (size_t)k);
}

// 5a. getFitness of every survivor: item = (survivor, chunk of 256 source points in stored order).  A point is an inlier iff the
// squared distance to its nearest target point, widened, is < max_d2.  The item's sum: a butterfly over each wave's 64 lanes, then
// the four waves in order.
__global__ __launch_bounds__(256) void prerej_score_kernel(CloudView src, BvhView tgt, const float *__restrict__ rows,
                                                            const uint32_t *__restrict__ d_nsurv, uint32_t chunks, double max_d2,
                                                            uint32_t *__restrict__ part_cnt, double *__restrict__ part_sum) {
  __shared__ float s_stk[kMaxDepth + 1][256];
  float *stk = &s_stk[0][threadIdx.x];
  const unsigned long long nitems = (unsigned long long)*d_nsurv * chunks;
  for (unsigned long long item = blockIdx.x; item < nitems; item += gridDim.x) {
    const uint32_t k = (uint32_t)(item / chunks), c = (uint32_t)(item % chunks);
    const float *F = rows + 12 * (size_t)k;
    const uint32_t i = c * 256 + threadIdx.x;
    double d = 0.0;
    bool in = false;
    if (i < src.n_valid) {
      const float4 s = src.xyzw[i];
      const float x = xform_row(F + 0, s.x, s.y, s.z);
      const float y = xform_row(F + 4, s.x, s.y, s.z);
      const float z = xform_row(F + 8, s.x, s.y, s.z);
      NearestVisitor v{INFINITY, kNoPos, 0};
      bvh_traverse(tgt, x, y, z, v, stk, 256);
      in = v.pos != kNoPos && (double)v.best < max_d2;
      if (in) d = (double)v.best;
    }
    item_sum(in, d, part_cnt + item, part_sum + item);
  }
}

// 5b. one lane per survivor: its partials in chunk order; error = sum / inliers, FLT_MAX without inliers
__global__ __launch_bounds__(kPrBlock) void prerej_reduce_kernel(const uint32_t *__restrict__ part_cnt, const double *__restrict__ part_sum,
                                                                 const uint32_t *__restrict__ d_nsurv, uint32_t chunks,
                                                                 int32_t *__restrict__ inliers, double *__restrict__ error) {
  const uint32_t k = blockIdx.x * kPrBlock + threadIdx.x;
  if (k >= *d_nsurv) return;
  survivor_sum(part_cnt, part_sum, k, chunks, inliers, error);
}

// 7. the inlier test of one transform, as flags by ORIGINAL index (non-finite points: 0)
__global__ __launch_bounds__(256) void prerej_inlier_kernel(CloudView src, BvhView tgt, const float *__restrict__ F, double max_d2,
                                                             uint8_t *__restrict__ flags_o) {
  __shared__ float s_stk[kMaxDepth + 1][256];
  float *stk = &s_stk[0][threadIdx.x];
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= src.n) return;
  const float4 s = src.xyzw[i];
  const uint32_t o = (uint32_t)__float_as_int(s.w);
  if (o >= src.n) return;
  bool in = false;
  if (i < src.n_valid) {
    const float x = xform_row(F + 0, s.x, s.y, s.z);
    const float y = xform_row(F + 4, s.x, s.y, s.z);
    const float z = xform_row(F + 8, s.x, s.y, s.z);
    NearestVisitor v{INFINITY, kNoPos, 0};
    bvh_traverse(tgt, x, y, z, v, stk, 256);
    in = v.pos != kNoPos && (double)v.best < max_d2;
  }
  flags_o[o] = in ? 1 : 0;
}

}  // namespace
}  // namespace ope

using namespace ope;

extern "C" {

void ope_prerejective_default_params(ope_prerejective_params *p) {
  if (!p) return;
  p->max_iterations = 50000;        /* BuildModel/src/poseestimator.cpp:97 */
  p->nr_samples = 3;                /* :98 */
  p->k_correspondences = 5;         /* :99 */
  p->similarity_threshold = 0.8f;   /* :100 */
  p->max_corr_dist = 0.15;          /* :101 */
  p->inlier_fraction = 0.25f;       /* :102 */
  p->seed = 1;
}

int ope_prerejective(ope_ctx *ctx, const ope_cloud *src, const float *src_feat33, const ope_cloud *tgt, const ope_index *tgt_index,
                     const float *tgt_feat33, const ope_prerejective_params *params, const int32_t *forced_samples,
                     ope_prerejective_result *out, int32_t *out_inliers) {
  static const char *who = "ope_prerejective: ";
  if (!ctx) return OPE_EINVAL;
  if (out) {
    std::memcpy(out->T, kIdentity4, sizeof kIdentity4);
    out->error = (double)FLT_MAX;
    out->best_iteration = -1;
    out->inliers = 0;
    out->converged = 0;
  }
  if (!src || !tgt || !tgt_index || !out || (!forced_samples && (!src_feat33 || !tgt_feat33)))
    return set_err(ctx, OPE_EINVAL, std::string(who) + "bad argument");
  ope_prerejective_params p;
  ope_prerejective_default_params(&p);
  if (params) p = *params;
  const int S = p.nr_samples, K = p.k_correspondences, H = p.max_iterations;
  if (const int rc = prerej_check_params(ctx, who, p)) return rc;
  if (tgt->n_valid == 0 || tgt_index->n == 0) return set_err(ctx, OPE_EINVAL, std::string(who) + "empty target (no finite point in the cloud or in the index)");
  if (src->n > (size_t)0x7fffffff || tgt->n > (size_t)0x7fffffff) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than 2^31 - 1 points");
  const int ns = (int)src->n, nt = (int)tgt->n;
  if (ns < S) return set_err(ctx, OPE_EINVAL, std::string(who) + "fewer source points than nr_samples");
  if (K > nt) return set_err(ctx, OPE_EINVAL, std::string(who) + "k_correspondences above the number of target points");
  if (const int rc = refuse_communicator(ctx, who)) return rc;
  const size_t HS = (size_t)H * S;
  if (forced_samples)
    for (size_t j = 0; j < HS; ++j)
      if (forced_samples[j] < 0 || forced_samples[j] >= ns || forced_samples[HS + j] < 0 || forced_samples[HS + j] >= nt)
        return set_err(ctx, OPE_EINVAL, std::string(who) + "sample index out of range");
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  TraceRange r_pr(ctx, "prerejective");
  ope_prerejective_stats &St = ctx->prerej_stats;
  St = ope_prerejective_stats{};
  St.iterations = H;
  St.nr_samples = S;
  ctx->prerej_samples.clear(); ctx->prerej_targets.clear(); ctx->prerej_survived.clear();
  ctx->prerej_T.clear(); ctx->prerej_inliers.clear(); ctx->prerej_error.clear();
  const hipStream_t st = ctx->stream;
  CallTmp tmp{st, {}};
  hipError_t e = hipSuccess;

  // ---- 2. draws (host) and the feature search (device)
  std::vector<int32_t> samp(HS), corr(HS);
  if (forced_samples) {
    std::memcpy(samp.data(), forced_samples, 4 * HS);
    std::memcpy(corr.data(), forced_samples + HS, 4 * HS);
  } else {
    std::vector<int32_t> pick(HS);
    prerej_draws(ns, S, K, H, p.seed, samp.data(), pick.data());
    std::vector<int32_t> slot((size_t)ns, -1), uniq;   // the distinct sampled source points, in order of first use
    for (int32_t s : samp)
      if (slot[(size_t)s] < 0) { slot[(size_t)s] = (int32_t)uniq.size(); uniq.push_back(s); }
    std::vector<float> qf(uniq.size() * 33);
    for (size_t u = 0; u < uniq.size(); ++u) std::memcpy(&qf[u * 33], src_feat33 + (size_t)uniq[u] * 33, 33 * sizeof(float));
    std::vector<int32_t> nn(uniq.size() * K);
    const size_t tf_bytes = sizeof(float) * 33 * (size_t)nt, qf_bytes = sizeof(float) * qf.size();
    auto *d_feat = (unsigned char *)tmp.get(tf_bytes + qf_bytes, e);
    auto *d_nn = (int32_t *)tmp.get(sizeof(int32_t) * nn.size(), e);
    const HostRange feats[2] = {{tgt_feat33, tf_bytes}, {qf.data(), qf_bytes}};
    if (e == hipSuccess) e = upload_staged(st, d_feat, feats, 2, &St.launches, &St.host_syncs);
    if (e == hipSuccess) {
      STAGE_LAUNCH(ctx, St.launches, prerej_feature_knn_kernel, 132.0 * ((double)uniq.size() * (double)nt + (double)uniq.size()), dim3((unsigned)uniq.size()),
                   dim3(256), 0, st, (const float *)d_feat, nt, (const float *)(d_feat + tf_bytes), K, d_nn);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(nn.data(), d_nn, sizeof(int32_t) * nn.size(), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    ++St.host_syncs;
    if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + "(feature search) " + hipGetErrorString(e));
    for (size_t j = 0; j < HS; ++j) {
      const int32_t *row = &nn[(size_t)slot[(size_t)samp[j]] * K];
      const int32_t c = row[pick[j]];
      corr[j] = c >= 0 ? c : row[0];
      if (corr[j] < 0 || corr[j] >= nt) return set_err(ctx, OPE_EINVAL, std::string(who) + "a sampled source descriptor has no finite neighbour");
    }
  }

  // ---- 1, 3. original order, the polygon test, the survivors in iteration order
  const size_t chunks = std::max<size_t>((src->n_valid + 255) / 256, 1);
  auto *src_o = (float4 *)tmp.get(16 * (size_t)ns, e);
  auto *tgt_o = (float4 *)tmp.get(16 * (size_t)nt, e);
  auto *d_pairs = (unsigned char *)tmp.get(8 * HS, e);
  auto *d_flags = (uint8_t *)tmp.get((size_t)H, e);
  auto *d_surv = (int32_t *)tmp.get(4 * (size_t)H, e);
  auto *d_nsurv = (uint32_t *)tmp.get(16, e);
  size_t tb = 0;
  if (e == hipSuccess) e = select_flagged_bytes(st, d_flags, d_surv, d_nsurv, (size_t)H, &tb);
  void *d_sel = tmp.get(std::max<size_t>(tb, 16), e);
  const HostRange pairs[2] = {{samp.data(), 4 * HS}, {corr.data(), 4 * HS}};
  if (e == hipSuccess) e = upload_staged(st, d_pairs, pairs, 2, &St.launches, &St.host_syncs);
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  const auto *d_samp = (const int32_t *)d_pairs, *d_corr = (const int32_t *)(d_pairs + 4 * HS);
  STAGE_LAUNCH(ctx, St.launches, prerej_orig_kernel, 32.0 * ns, dim3(grid_of(ns, kPrBlock)), dim3(kPrBlock), 0, st, src->view(), src_o);
  STAGE_LAUNCH(ctx, St.launches, prerej_orig_kernel, 32.0 * nt, dim3(grid_of(nt, kPrBlock)), dim3(kPrBlock), 0, st, tgt->view(), tgt_o);
  const float thr2 = p.similarity_threshold * p.similarity_threshold;
  STAGE_LAUNCH(ctx, St.launches, prerej_polygon_kernel, (double)H * (40.0 * S + 1.0), dim3(grid_of(H, kPrBlock)), dim3(kPrBlock), 0, st, src_o, tgt_o, d_samp,
               d_corr, (uint32_t)H, S, thr2, d_flags);
  e = select_flagged(ctx, "prerej_select", 5.0 * H, &St.launches, d_sel, tb, d_flags, d_surv, d_nsurv, (size_t)H);
  uint32_t nsurv = 0;
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(&nsurv, d_nsurv, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  ++St.host_syncs;
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + "(prerejection) " + hipGetErrorString(e));
  nsurv = std::min(nsurv, (uint32_t)H);
  St.survivors = nsurv;

  // ---- 4, 5. fits and scores of the survivors
  const size_t ns1 = std::max<size_t>(nsurv, 1), nitems = ns1 * chunks;
  auto *d_T = (float *)tmp.get(64 * ns1, e);
  auto *d_rows = (float *)tmp.get(48 * ns1, e);
  auto *d_pcnt = (uint32_t *)tmp.get(4 * nitems, e);
  auto *d_psum = (double *)tmp.get(8 * nitems, e);
  auto *d_inl = (int32_t *)tmp.get(4 * ns1, e);
  auto *d_err = (double *)tmp.get(8 * ns1, e);
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  const double max_d2 = p.max_corr_dist * p.max_corr_dist;
  STAGE_LAUNCH(ctx, St.launches, prerej_fit_kernel, (double)nsurv * (40.0 * S + 112.0), dim3(grid_of(nsurv, 64)), dim3(64), 0, st, src_o, tgt_o, d_samp, d_corr,
               S, d_surv, d_nsurv, d_T, d_rows);
  const unsigned score_blocks = (unsigned)std::min<size_t>(nitems, (size_t)ctx->n_cu * 16);
  STAGE_LAUNCH(ctx, St.launches, prerej_score_kernel, 24.0 * (double)src->n_valid * (double)nsurv, dim3(score_blocks), dim3(256), 0, st, src->view(),
               tgt_index->view(), d_rows, d_nsurv, (uint32_t)chunks, max_d2, d_pcnt, d_psum);
  STAGE_LAUNCH(ctx, St.launches, prerej_reduce_kernel, 12.0 * (double)nitems, dim3(grid_of(nsurv, kPrBlock)), dim3(kPrBlock), 0, st, d_pcnt, d_psum, d_nsurv,
               (uint32_t)chunks, d_inl, d_err);
  std::vector<uint8_t> flags((size_t)H);
  std::vector<int32_t> surv(ns1), inl(ns1);
  std::vector<float> Ts(16 * ns1);
  std::vector<double> err(ns1);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(flags.data(), d_flags, (size_t)H, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && nsurv) e = hipMemcpyAsync(surv.data(), d_surv, 4 * (size_t)nsurv, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && nsurv) e = hipMemcpyAsync(Ts.data(), d_T, 64 * (size_t)nsurv, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && nsurv) e = hipMemcpyAsync(inl.data(), d_inl, 4 * (size_t)nsurv, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && nsurv) e = hipMemcpyAsync(err.data(), d_err, 8 * (size_t)nsurv, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  ++St.host_syncs;
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + "(fitness) " + hipGetErrorString(e));

  // ---- 6. the accept loop, replayed in iteration order (survivors are in iteration order)
  const int64_t best = prerej_accept(inl.data(), err.data(), nsurv, ns, p.inlier_fraction);
  ctx->prerej_samples = samp;
  ctx->prerej_targets = corr;
  ctx->prerej_survived = flags;
  ctx->prerej_T.resize(16 * (size_t)H);
  ctx->prerej_inliers.assign((size_t)H, 0);
  ctx->prerej_error.assign((size_t)H, (double)FLT_MAX);
  for (int it = 0; it < H; ++it) std::memcpy(&ctx->prerej_T[16 * (size_t)it], kIdentity4, sizeof kIdentity4);
  for (uint32_t k = 0; k < nsurv; ++k) {
    const size_t it = (size_t)surv[k];
    if (it >= (size_t)H) return set_err(ctx, OPE_EHIP, std::string(who) + "a survivor's iteration is out of range");
    std::memcpy(&ctx->prerej_T[16 * it], &Ts[16 * (size_t)k], 64);
    ctx->prerej_inliers[it] = inl[k];
    ctx->prerej_error[it] = err[k];
  }
  if (best >= 0) {
    std::memcpy(out->T, &Ts[16 * (size_t)best], 64);
    out->error = err[best];
    out->best_iteration = surv[best];
    out->inliers = inl[best];
    out->converged = 1;
  }

  // ---- 7. the winner's inliers (without a winner the pass still runs, on the identity, and its result is dropped)
  if (out_inliers) {
    float rows[12];
    colmajor_to_rows12(out->T, rows);
    auto *d_wrows = (float *)tmp.get(48, e);
    auto *d_fo = (uint8_t *)tmp.get((size_t)ns, e);
    auto *d_idx = (int32_t *)tmp.get(4 * (size_t)ns, e);
    auto *d_cnt = (uint32_t *)tmp.get(16, e);
    size_t tb2 = 0;
    if (e == hipSuccess) e = select_flagged_bytes(st, d_fo, d_idx, d_cnt, (size_t)ns, &tb2);
    void *d_sel2 = tmp.get(std::max<size_t>(tb2, 16), e);
    if (e == hipSuccess) { e = h2d_copy(st, d_wrows, rows, 48); ++St.launches; }
    if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
    STAGE_LAUNCH(ctx, St.launches, prerej_inlier_kernel, 24.0 * (double)src->n_valid, dim3(grid_of(ns, 256)), dim3(256), 0, st, src->view(), tgt_index->view(),
                 d_wrows, max_d2, d_fo);
    e = select_flagged(ctx, "prerej_select", 5.0 * ns, &St.launches, d_sel2, tb2, d_fo, d_idx, d_cnt, (size_t)ns);
    uint32_t cnt = 0;
    std::vector<int32_t> idx((size_t)ns);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&cnt, d_cnt, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(idx.data(), d_idx, 4 * (size_t)ns, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    ++St.host_syncs;
    if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + "(inliers) " + hipGetErrorString(e));
    if (best >= 0) {
      if ((int64_t)cnt != (int64_t)out->inliers) return set_err(ctx, OPE_EHIP, std::string(who) + "the winner's inlier list and its count disagree");
      std::memcpy(out_inliers, idx.data(), 4 * (size_t)cnt);
    }
  }
  return OPE_OK;
}

int ope_prerejective_last_stats(const ope_ctx *ctx, ope_prerejective_stats *out) {
  if (!ctx || !out) return OPE_EINVAL;
  *out = ctx->prerej_stats;
  return OPE_OK;
}

int ope_prerejective_last_hypotheses(const ope_ctx *ctx, int32_t *samples, int32_t *targets, uint8_t *survived, float *T, int32_t *inliers,
                                     double *error, size_t cap, size_t *n_out) {
  if (!ctx || !n_out) return OPE_EINVAL;
  const size_t made = ctx->prerej_survived.size(), w = std::min(made, cap), S = (size_t)ctx->prerej_stats.nr_samples;
  if (samples && w) std::memcpy(samples, ctx->prerej_samples.data(), 4 * S * w);
  if (targets && w) std::memcpy(targets, ctx->prerej_targets.data(), 4 * S * w);
  if (survived && w) std::memcpy(survived, ctx->prerej_survived.data(), w);
  if (T && w) std::memcpy(T, ctx->prerej_T.data(), 64 * w);
  if (inliers && w) std::memcpy(inliers, ctx->prerej_inliers.data(), 4 * w);
  if (error && w) std::memcpy(error, ctx->prerej_error.data(), 8 * w);
  *n_out = made;
  return OPE_OK;
}

}  // extern "C"
