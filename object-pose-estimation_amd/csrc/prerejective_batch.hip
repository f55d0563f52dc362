// prerejective_batch.hip — estimateCoarsePose with the prerejective aligner for one model and many candidate clusters in one call
// (ope_prerejective_pose_batch, gfx950, wave64).  DESIGN.md §4.21 has the float order of every step.
//
// The single path pays per cluster its own sampling, normals, FPFH, upload, index build and one ope_prerejective (10 launches,
// 3 synchronisations, 8 bytes per draw uploaded).  Here every stage runs once for all clusters:
//   a. the front end of ope_coarse_pose_batch (coarse_front_launch: key points, normals, FPFH of the model and every cluster);
//   b. the host draws every active cluster's iterations by ope_prerejective's loop (prerej_draws) while the device computes the
//      features; they go up packed, 16 bits per draw (sample | pick << 12), in one copy.  With ope_prerejective_set_draws(ctx,
//      OPE_DRAWS_DEVICE) the same words are written in place by prerejective_draws.hip (a seed upload and three launches: 12
//      launches for the call instead of 9); a problem the device could not finish comes back with the second synchronisation, is
//      drawn here and uploaded, and d, e run again;
//   c. one launch finds the k nearest descriptors of every model key point in every active cluster (feature_knn_block); the rows
//      stay on the device;
//   d. one lane per (cluster, iteration) turns picks into targets and runs the polygon test (polygon_ok); a sampled row without a
//      finite neighbour sets the cluster's NaN word;
//   e. one rocPRIM select over all flags, cluster-major: the survivors in (cluster, iteration) order; one lane per cluster finds its
//      first survivor by binary search; the total and the offsets come back (second synchronisation, the first is the front end's);
//   f. one lane per survivor fits Umeyama in fp64 (umeyama_fit);
//   g. one work item per (survivor, 256 model key points in KEY-POINT order): the cluster's key points staged in LDS, brute-force
//      exact 1-NN, the item's count and fp64 sum by item_sum; one lane per survivor adds its partials in chunk order;
//   h. the survivors' transforms, counts and errors come back (third synchronisation); the host replays the accept loop per cluster.
// Neither the launches nor the synchronisations depend on the clusters, the iterations, the survivors or the points; nothing is
// summed across clusters, and the order of a sum depends on the model's key points alone.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "coarse_stages.hpp"
#include "feature_math.hpp"
#include "prerejective_draws_plan.hpp"
#include "prerejective_math.hpp"
#include "stage_host.hpp"

namespace ope {
namespace {

// what the kernels of one call read: segment 0 of kp / fpfh is the model, active[a].x the segment of active cluster a
struct PbView {
  const float4 *kp;           // key points packed by segment
  const uint32_t *key_off;    // nseg + 1
  const int2 *active;         // na
  const uint16_t *draws;      // na * H * S: sample | pick << 12
  const int32_t *nn;          // na * nsk * K: the feature rows
  uint32_t H, nsk;
  int S, K;
};

// the i-th pair of iteration `it` of active cluster a (t0 = the cluster's first key slot): the target is the pick-th entry of the
// sample's row, or row[0] when that entry is -1; a row without any entry sets bad (and hands out the cluster's first key point)
__device__ __forceinline__ void pb_pair(const PbView &v, uint32_t a, uint32_t it, uint32_t t0, int i, float4 &s, float4 &t, bool &bad) {
  const uint32_t w = v.draws[((size_t)a * v.H + it) * v.S + i];
  const uint32_t sm = w & 0xfffu, pk = (w >> 12) & 7u;
  const int32_t *row = v.nn + ((size_t)a * v.nsk + sm) * v.K;
  int32_t c = row[pk];
  if (c < 0) c = row[0];
  if (c < 0) { bad = true; c = 0; }
  s = v.kp[v.key_off[0] + sm];
  t = v.kp[t0 + (uint32_t)c];
}

// c. findSimilarFeatures: block (u, a) = model key point u against the descriptors of active cluster a
__global__ __launch_bounds__(256) void prerej_batch_knn_kernel(const float *__restrict__ fpfh, const uint32_t *__restrict__ key_off,
                                                                const int2 *__restrict__ active, int k, int32_t *__restrict__ out_idx) {
  const uint32_t t0 = key_off[active[blockIdx.y].x], nt = key_off[active[blockIdx.y].x + 1] - t0;
  const size_t u = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  feature_knn_block(fpfh + (size_t)t0 * 33, (int)nt, fpfh + (size_t)(key_off[0] + blockIdx.x) * 33, k, out_idx + u * k);
}

// d. one lane per (cluster, iteration), cluster-major
__global__ __launch_bounds__(kPrBlock) void prerej_batch_polygon_kernel(PbView v, uint32_t total, float thr2, uint8_t *__restrict__ flags,
                                                                        uint32_t *__restrict__ nan_word) {
  const uint32_t g = blockIdx.x * kPrBlock + threadIdx.x;
  if (g >= total) return;
  const uint32_t a = g / v.H, it = g - a * v.H, t0 = v.key_off[v.active[a].x];
  bool bad = false;
  const bool ok = polygon_ok(v.S, thr2, [&](int i, float4 &s, float4 &t) { pb_pair(v, a, it, t0, i, s, t, bad); });
  flags[g] = (ok && !bad) ? 1 : 0;
  if (bad) atomicOr(nan_word + a, 1u);
}

// e. first survivor of every active cluster (na + 1 entries): the survivors are ascending in cluster * H + iteration
__global__ __launch_bounds__(kPrBlock) void prerej_batch_offsets_kernel(const uint32_t *__restrict__ surv, const uint32_t *__restrict__ d_nsurv,
                                                                        uint32_t na, uint32_t H, uint32_t *__restrict__ off) {
  const uint32_t a = blockIdx.x * kPrBlock + threadIdx.x;
  if (a > na) return;
  const unsigned long long first = (unsigned long long)a * H;
  uint32_t lo = 0, hi = *d_nsurv;   // first k with surv[k] >= first
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if ((unsigned long long)surv[mid] < first) lo = mid + 1; else hi = mid;
  }
  off[a] = lo;
}

// f. one lane per survivor
__global__ __launch_bounds__(64) void prerej_batch_fit_kernel(PbView v, const uint32_t *__restrict__ surv, uint32_t nsurv,
                                                              float *__restrict__ T_out, float *__restrict__ rows_out) {
  const uint32_t k = blockIdx.x * 64 + threadIdx.x;
  if (k >= nsurv) return;
  const uint32_t g = surv[k], a = g / v.H, it = g - a * v.H, t0 = v.key_off[v.active[a].x];
  bool bad = false;
  umeyama_fit(v.S, [&](int i, float4 &s, float4 &t) { pb_pair(v, a, it, t0, i, s, t, bad); }, T_out + 16 * (size_t)k, rows_out + 12 * (size_t)k);
}

// g. getFitness: item = (survivor, chunk of 256 model key points in key-point order).  A point is an inlier iff the squared distance
// to its nearest cluster key point (brute force over the cluster's key points in LDS), widened, is < max_d2.
__global__ __launch_bounds__(256) void prerej_batch_score_kernel(PbView v, const uint32_t *__restrict__ surv, const float *__restrict__ rows,
                                                                  unsigned long long nitems, uint32_t chunks, double max_d2,
                                                                  uint32_t *__restrict__ part_cnt, double *__restrict__ part_sum) {
  extern __shared__ float4 s_pts[];
  for (unsigned long long item = blockIdx.x; item < nitems; item += gridDim.x) {
    const uint32_t k = (uint32_t)(item / chunks), c = (uint32_t)(item % chunks);
    const uint32_t a = surv[k] / v.H, seg = (uint32_t)v.active[a].x, t0 = v.key_off[seg], nt = v.key_off[seg + 1] - t0;
    for (uint32_t j = threadIdx.x; j < nt; j += 256) s_pts[j] = v.kp[t0 + j];
    __syncthreads();
    const float *F = rows + 12 * (size_t)k;
    const uint32_t i = c * 256 + threadIdx.x;
    double d = 0.0;
    bool in = false;
    if (i < v.nsk) {
      const float4 s = v.kp[v.key_off[0] + i];
      const float x = xform_row(F + 0, s.x, s.y, s.z);
      const float y = xform_row(F + 4, s.x, s.y, s.z);
      const float z = xform_row(F + 8, s.x, s.y, s.z);
      float best = INFINITY;
#pragma unroll 4
      for (uint32_t t = 0; t < nt; ++t) {
        const float4 P = s_pts[t];
        best = fminf(best, sq_dist3(__fsub_rn(x, P.x), __fsub_rn(y, P.y), __fsub_rn(z, P.z)));
      }
      in = (double)best < max_d2;
      if (in) d = (double)best;
    }
    item_sum(in, d, part_cnt + item, part_sum + item);   // (ends with a barrier: the next item may restage)
  }
}

__global__ __launch_bounds__(kPrBlock) void prerej_batch_reduce_kernel(const uint32_t *__restrict__ part_cnt, const double *__restrict__ part_sum,
                                                                       uint32_t nsurv, uint32_t chunks, int32_t *__restrict__ inliers,
                                                                       double *__restrict__ error) {
  const uint32_t k = blockIdx.x * kPrBlock + threadIdx.x;
  if (k >= nsurv) return;
  survivor_sum(part_cnt, part_sum, k, chunks, inliers, error);
}

}  // namespace

int prerejective_pose_batch_impl(ope_ctx *ctx, const char *who, const ope_cloud *model, size_t n, const ope_cloud *const *clusters,
                                 const ope_coarse_params *front, const ope_prerejective_params *params, const uint64_t *seeds,
                                 bool seed_by_rank, int keep_hypotheses, ope_prerejective_batch_result *out) {
  if (!ctx) return OPE_EINVAL;
  if (n == 0) return OPE_OK;
  if (!model || !clusters || !out) return set_err(ctx, OPE_EINVAL, std::string(who) + "bad argument");
  if (n > 65535) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than 65535 clusters (one grid row each)");
  ope_coarse_params fp;
  ope_coarse_default_params(&fp);
  if (front) fp = *front;
  ope_prerejective_params p;
  ope_prerejective_default_params(&p);
  if (params) p = *params;
  const int S = p.nr_samples, K = p.k_correspondences, H = p.max_iterations;
  if (const int rc = prerej_check_params(ctx, who, p)) return rc;
  if ((unsigned long long)n * (unsigned long long)H > 0x7fffffffull)
    return set_err(ctx, OPE_EINVAL, std::string(who) + "clusters x max_iterations above 2^31 - 1");
  if (const int rc = refuse_communicator(ctx, who)) return rc;
  if (ctx->draws_mode == OPE_DRAWS_DEVICE && ctx->draws_window && ctx->draws_window < 2 * S)
    return set_err(ctx, OPE_EINVAL, std::string(who) + "the draws' window (ope_prerejective_set_draws_limits) is below 2 * nr_samples");
  // the front end's refusals (sizes, key points; the model needs nr_samples key points)
  fp.sacia.nr_samples = S; fp.sacia.k_correspondences = K; fp.sacia.max_iterations = H;
  long long model_keys = -2;
  { const int rc = coarse_batch_check(ctx, model, n, clusters, fp, &model_keys, who); if (rc != OPE_OK) return rc; }

  OPE_HIP(ctx, hipSetDevice(ctx->device));
  TraceRange r_all(ctx, "prerejective_batch");
  ope_prerejective_batch_stats &St = ctx->pb_stats;
  St = ope_prerejective_batch_stats{};
  St.clusters = (int64_t)n;
  St.iterations = H;
  St.nr_samples = S;
  ctx->pb_hyp_off.clear(); ctx->pb_surv_off.clear();
  ctx->pb_samples.clear(); ctx->pb_targets.clear(); ctx->pb_survived.clear();
  ctx->pb_surv_it.clear(); ctx->pb_surv_inl.clear(); ctx->pb_surv_T.clear(); ctx->pb_surv_err.clear();
  const hipStream_t st = ctx->stream;
  CallTmp tmp{st, {}};
  hipError_t e = hipSuccess;
  auto fail = [&](const char *what) { return set_err(ctx, OPE_EHIP, std::string(who) + what + ": " + hipGetErrorString(e)); };

  // ---- a. the front end (first synchronisation: the key offsets)
  CoarseFront fr;
  { const int rc = coarse_front_launch(ctx, tmp, who, model, n, clusters, fp, model_keys, fr); if (rc != OPE_OK) return rc; }
  ++St.host_syncs;
  const std::vector<uint32_t> &key_off = fr.key_off;
  const uint32_t nsk = fr.nsk;
  std::vector<int2> active;
  std::vector<size_t> active_cluster;
  for (size_t i = 0; i < n; ++i) {
    ope_prerejective_batch_result &o = out[i];
    std::memset(&o, 0, sizeof o);
    std::memcpy(o.T, kIdentity4, sizeof kIdentity4);
    o.error = (double)FLT_MAX;
    o.best_iteration = -1;
    o.n_src_keys = (int32_t)nsk;
    o.n_tgt_keys = (int32_t)(key_off[i + 2] - key_off[i + 1]);
    o.status = clusters[i]->n == 0 ? OPE_PREREJ_EMPTY_TARGET : o.n_tgt_keys < 10 ? OPE_PREREJ_FEW_TARGET_FEATURES : OPE_PREREJ_OK;
    if (o.status == OPE_PREREJ_OK) { active.push_back(make_int2((int)(i + 1), 0)); active_cluster.push_back(i); }
  }
  const size_t na = active.size();
  St.active = (int64_t)na;
  if (na == 0) {
    e = coarse_front_download(ctx, fr);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    ++St.host_syncs;
    if (e != hipSuccess) return fail("download");
    coarse_front_keep(ctx, fr);
    return OPE_OK;
  }

  // ---- b. the draws of every active cluster (the device computes the features meanwhile), packed
  TraceRange r_al(ctx, "prerejective_batch_align");
  const size_t HS = (size_t)H * S, total = na * (size_t)H;
  std::vector<uint64_t> seed_of(na);
  for (size_t a = 0; a < na; ++a) seed_of[a] = seeds ? seeds[active_cluster[a]] : p.seed + (uint64_t)(seed_by_rank ? a : active_cluster[a]);
  // with OPE_DRAWS_DEVICE the draws are made in place by prerejective_draws.hip, unless their tile tables are too large for one call
  const bool want_device = ctx->draws_mode == OPE_DRAWS_DEVICE;
  const DrawPlan plan = draw_plan((int)nsk, S, H, na, want_device ? ctx->draws_window : 0, want_device ? ctx->draws_budget : 0);
  const bool device_draws = want_device && plan.fits;
  draw_stats_begin(ctx->draws_stats, ctx->draws_mode, plan, device_draws);
  // the host's copies of the draws: all of them with host draws; with device draws only for a fallback or the kept hypotheses
  std::vector<uint16_t> draws;
  std::vector<int32_t> samp, pick;
  if (!device_draws) draws.resize(na * HS);
  if (keep_hypotheses) ctx->pb_samples.resize(na * HS);
  auto host_draws = [&](size_t a) {
    draws.resize(na * HS);
    samp.resize(HS); pick.resize(HS);
    prerej_draws((int)nsk, S, K, H, seed_of[a], samp.data(), pick.data());
    uint16_t *w = &draws[a * HS];
    for (size_t j = 0; j < HS; ++j) w[j] = (uint16_t)((uint32_t)samp[j] | ((uint32_t)pick[j] << 12));
    if (keep_hypotheses) std::memcpy(&ctx->pb_samples[a * HS], samp.data(), 4 * HS);
  };
  if (!device_draws)
    for (size_t a = 0; a < na; ++a) host_draws(a);

  const size_t draw_bytes = 2 * na * HS;
  auto *d_active = (int2 *)tmp.get(sizeof(int2) * na, e);
  auto *d_draws = (uint16_t *)tmp.get(draw_bytes, e);
  auto *d_nn = (int32_t *)tmp.get(4 * na * (size_t)nsk * K, e);
  auto *d_flags = (uint8_t *)tmp.get(total, e);
  auto *d_surv = (uint32_t *)tmp.get(4 * total, e);
  auto *d_words = (uint32_t *)tmp.get(4 * (2 * na + 2), e);   // [nsurv | off (na + 1) | NaN words (na)]
  size_t tb = 0;
  if (e == hipSuccess) e = select_flagged_bytes(st, d_flags, d_surv, d_words, total, &tb);
  void *d_sel = tmp.get(std::max<size_t>(tb, 16), e);
  if (e == hipSuccess) e = h2d_copy(st, d_active, active.data(), sizeof(int2) * na);
  if (e != hipSuccess) return fail("buffers");
  uint32_t *d_nsurv = d_words, *d_off = d_words + 1, *d_nan = d_words + 2 + na;
  uint32_t *d_draw_words = nullptr;   // device draws: per problem, whether the host has to draw it after all
  if (device_draws) {
    const int64_t before = St.launches;
    e = draws_device_launch(ctx, tmp, plan, (int)nsk, S, K, H, seed_of.data(), na, d_draws, &d_draw_words, &St.launches, &St.host_syncs);
    ctx->draws_stats[kDsLaunches] = St.launches - before;
  } else {
    e = upload_staged(st, d_draws, draws.data(), draw_bytes, &St.launches, &St.host_syncs);   // (nothing stages again before the next synchronisation)
  }
  if (e == hipSuccess) { e = hipMemsetAsync(d_nan, 0, 4 * na, st); ++St.launches; }
  if (e != hipSuccess) return fail("upload");

  // ---- c, d, e. feature rows, polygon test, survivors in (cluster, iteration) order and every cluster's first
  const PbView v{fr.d_kp, fr.d_key_off, d_active, d_draws, d_nn, (uint32_t)H, nsk, S, K};
  STAGE_LAUNCH(ctx, St.launches, prerej_batch_knn_kernel, 132.0 * (double)na * (double)nsk * (double)fr.max_keys, dim3(nsk, (unsigned)na), dim3(256), 0, st,
               (const float *)fr.d_fpfh, (const uint32_t *)fr.d_key_off, (const int2 *)d_active, K, d_nn);
  const float thr2 = p.similarity_threshold * p.similarity_threshold;
  std::vector<uint32_t> words(2 * na + 2), draw_words(device_draws ? na : 0);
  // d, e and the second synchronisation; first: the features and the draws' words come back with it
  auto prereject = [&](bool first) -> int {
    STAGE_LAUNCH(ctx, St.launches, prerej_batch_polygon_kernel, (double)total * (38.0 * S + 1.0), dim3(grid_of(total, kPrBlock)), dim3(kPrBlock), 0, st, v,
                 (uint32_t)total, thr2, d_flags, d_nan);
    e = select_flagged(ctx, "prerej_batch_select", 5.0 * (double)total, &St.launches, d_sel, tb, d_flags, d_surv, d_nsurv, total);
    if (e != hipSuccess) return fail("select");
    STAGE_LAUNCH(ctx, St.launches, prerej_batch_offsets_kernel, 8.0 * (double)na, dim3(grid_of(na + 1, kPrBlock)), dim3(kPrBlock), 0, st,
                 (const uint32_t *)d_surv, (const uint32_t *)d_nsurv, (uint32_t)na, (uint32_t)H, d_off);
    e = hipGetLastError();
    if (e == hipSuccess && first) e = coarse_front_download(ctx, fr);
    if (e == hipSuccess) e = hipMemcpyAsync(words.data(), d_words, 4 * words.size(), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && first && device_draws) e = hipMemcpyAsync(draw_words.data(), d_draw_words, 4 * na, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    ++St.host_syncs;
    if (e != hipSuccess) return fail("prerejection");
    return OPE_OK;
  };
  if (const int rc = prereject(true)) return rc;
  if (device_draws) {
    // a problem the device could not finish is drawn here, goes up into its slice, and the prerejection runs again
    const std::vector<size_t> again = draw_fallbacks(draw_words.data(), na, ctx->draws_stats);
    for (const size_t a : again) {
      host_draws(a);
      e = upload_staged(st, d_draws + a * HS, &draws[a * HS], 2 * HS, &St.launches, &St.host_syncs);
      if (e == hipSuccess) e = hipStreamSynchronize(st);   // (the staging block is filled again by the next problem)
      ++St.host_syncs;
      if (e != hipSuccess) return fail("upload");
    }
    if (!again.empty()) {
      e = hipMemsetAsync(d_nan, 0, 4 * na, st);
      ++St.launches;
      if (e != hipSuccess) return fail("upload");
      if (const int rc = prereject(false)) return rc;
    }
  }
  coarse_front_keep(ctx, fr);
  const uint32_t nsurv = std::min<uint32_t>(words[0], (uint32_t)total);
  const uint32_t *off = &words[1], *nan_word = &words[2 + na];
  St.survivors = nsurv;
  for (size_t a = 0; a <= na; ++a)
    if (off[a] > nsurv || (a && off[a] < off[a - 1])) return set_err(ctx, OPE_EHIP, std::string(who) + "the survivors' offsets are out of order");

  // ---- f, g. fits and scores of the survivors
  const size_t chunks = ((size_t)nsk + 255) / 256, ns1 = std::max<size_t>(nsurv, 1), nitems = (size_t)nsurv * chunks;
  auto *d_T = (float *)tmp.get(64 * ns1, e);
  auto *d_rows = (float *)tmp.get(48 * ns1, e);
  auto *d_pcnt = (uint32_t *)tmp.get(4 * std::max<size_t>(nitems, 1), e);
  auto *d_psum = (double *)tmp.get(8 * std::max<size_t>(nitems, 1), e);
  auto *d_inl = (int32_t *)tmp.get(4 * ns1, e);
  auto *d_err = (double *)tmp.get(8 * ns1, e);
  const size_t lds = 16 * (size_t)fr.max_keys;
  if (e == hipSuccess) e = hipFuncSetAttribute((const void *)prerej_batch_score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return fail("buffers");
  const double max_d2 = p.max_corr_dist * p.max_corr_dist;
  STAGE_LAUNCH(ctx, St.launches, prerej_batch_fit_kernel, (double)nsurv * (38.0 * S + 112.0), dim3(grid_of(nsurv, 64)), dim3(64), 0, st, v,
               (const uint32_t *)d_surv, nsurv, d_T, d_rows);
  const unsigned score_blocks = (unsigned)std::min<size_t>(std::max<size_t>(nitems, 1), (size_t)1 << 30);
  STAGE_LAUNCH(ctx, St.launches, prerej_batch_score_kernel, 16.0 * (double)nsk * (double)nsurv, dim3(score_blocks), dim3(256), lds, st, v,
               (const uint32_t *)d_surv, (const float *)d_rows, (unsigned long long)nitems, (uint32_t)chunks, max_d2, d_pcnt, d_psum);
  STAGE_LAUNCH(ctx, St.launches, prerej_batch_reduce_kernel, 12.0 * (double)nitems, dim3(grid_of(nsurv, kPrBlock)), dim3(kPrBlock), 0, st,
               (const uint32_t *)d_pcnt, (const double *)d_psum, nsurv, (uint32_t)chunks, d_inl, d_err);
  std::vector<uint32_t> surv(ns1);
  std::vector<int32_t> inl(ns1);
  std::vector<float> Ts(16 * ns1);
  std::vector<double> err(ns1);
  std::vector<int32_t> nn;
  e = hipGetLastError();
  if (e == hipSuccess && nsurv) e = hipMemcpyAsync(surv.data(), d_surv, 4 * (size_t)nsurv, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && nsurv) e = hipMemcpyAsync(Ts.data(), d_T, 64 * (size_t)nsurv, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && nsurv) e = hipMemcpyAsync(inl.data(), d_inl, 4 * (size_t)nsurv, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && nsurv) e = hipMemcpyAsync(err.data(), d_err, 8 * (size_t)nsurv, hipMemcpyDeviceToHost, st);
  if (keep_hypotheses) {
    ctx->pb_survived.resize(total);
    nn.resize(na * (size_t)nsk * K);
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->pb_survived.data(), d_flags, total, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(nn.data(), d_nn, 4 * nn.size(), hipMemcpyDeviceToHost, st);
    if (device_draws) draws.resize(na * HS);
    if (e == hipSuccess && device_draws) e = hipMemcpyAsync(draws.data(), d_draws, draw_bytes, hipMemcpyDeviceToHost, st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  ++St.host_syncs;
  if (e != hipSuccess) return fail("fitness");
  if (keep_hypotheses && device_draws)
    for (size_t j = 0; j < na * HS; ++j) ctx->pb_samples[j] = (int32_t)(draws[j] & 0xfffu);

  // ---- h. the accept loop per cluster, over its survivors in iteration order
  for (size_t a = 0; a < na; ++a) {
    ope_prerejective_batch_result &o = out[active_cluster[a]];
    if (nan_word[a]) { o.status = OPE_PREREJ_NAN_FEATURES; continue; }
    const size_t k0 = off[a], cnt = off[a + 1] - off[a];
    o.seed = seed_of[a];
    o.survivors = (int32_t)cnt;
    const int64_t best = prerej_accept(&inl[k0], &err[k0], cnt, (int)nsk, p.inlier_fraction);
    if (best < 0) continue;
    const size_t k = k0 + (size_t)best;
    std::memcpy(o.T, &Ts[16 * k], 64);
    o.error = err[k];
    o.best_iteration = (int32_t)(surv[k] - (uint32_t)(a * (size_t)H));
    o.inliers = inl[k];
    o.converged = 1;
  }
  if (keep_hypotheses) {
    ctx->pb_hyp_off.assign(n + 1, 0);
    ctx->pb_surv_off.assign(n + 1, 0);
    for (size_t i = 0, a = 0; i < n; ++i) {
      const bool act = a < na && active_cluster[a] == i;
      ctx->pb_hyp_off[i + 1] = ctx->pb_hyp_off[i] + (act ? (size_t)H : 0);
      ctx->pb_surv_off[i + 1] = act ? off[a + 1] : ctx->pb_surv_off[i];
      if (act) ++a;
    }
    ctx->pb_targets.resize(na * HS);
    for (size_t a = 0; a < na; ++a)
      for (size_t j = 0; j < HS; ++j) {
        const uint32_t w = draws[a * HS + j];
        const int32_t *row = &nn[(a * nsk + (w & 0xfffu)) * K];
        const int32_t c = row[(w >> 12) & 7u];
        ctx->pb_targets[a * HS + j] = c >= 0 ? c : row[0];
      }
    ctx->pb_surv_it.resize(nsurv);
    for (size_t a = 0; a < na; ++a)
      for (uint32_t k = off[a]; k < off[a + 1]; ++k) ctx->pb_surv_it[k] = (int32_t)(surv[k] - (uint32_t)(a * (size_t)H));
    ctx->pb_surv_inl.assign(inl.begin(), inl.begin() + nsurv);
    ctx->pb_surv_T.assign(Ts.begin(), Ts.begin() + 16 * (size_t)nsurv);
    ctx->pb_surv_err.assign(err.begin(), err.begin() + nsurv);
  }
  return OPE_OK;
}

}  // namespace ope

using namespace ope;

extern "C" {

int ope_prerejective_pose_batch(ope_ctx *ctx, const ope_cloud *model, size_t n, const ope_cloud *const *clusters, const ope_coarse_params *front,
                                const ope_prerejective_params *params, const uint64_t *seeds, int keep_hypotheses,
                                ope_prerejective_batch_result *out) {
  return prerejective_pose_batch_impl(ctx, "ope_prerejective_pose_batch: ", model, n, clusters, front, params, seeds, false, keep_hypotheses, out);
}

int ope_prerejective_batch_last_stats(const ope_ctx *ctx, ope_prerejective_batch_stats *out) {
  if (!ctx || !out) return OPE_EINVAL;
  *out = ctx->pb_stats;
  return OPE_OK;
}

int ope_prerejective_batch_hypotheses(const ope_ctx *ctx, int which, int32_t *samples, int32_t *targets, uint8_t *survived, float *T,
                                      int32_t *inliers, double *error, size_t cap, size_t *n_out) {
  if (!ctx || !n_out) return OPE_EINVAL;
  *n_out = 0;
  if (ctx->pb_hyp_off.empty() || which < 0 || (size_t)which + 1 >= ctx->pb_hyp_off.size()) return OPE_EINVAL;
  const size_t h0 = ctx->pb_hyp_off[(size_t)which], made = ctx->pb_hyp_off[(size_t)which + 1] - h0, w = std::min(made, cap);
  const size_t S = (size_t)ctx->pb_stats.nr_samples;
  if (samples && w) std::memcpy(samples, ctx->pb_samples.data() + S * h0, 4 * S * w);
  if (targets && w) std::memcpy(targets, ctx->pb_targets.data() + S * h0, 4 * S * w);
  if (survived && w) std::memcpy(survived, ctx->pb_survived.data() + h0, w);
  for (size_t it = 0; it < w; ++it) {
    if (T) std::memcpy(T + 16 * it, kIdentity4, sizeof kIdentity4);
    if (inliers) inliers[it] = 0;
    if (error) error[it] = (double)FLT_MAX;
  }
  for (size_t k = ctx->pb_surv_off[(size_t)which]; k < ctx->pb_surv_off[(size_t)which + 1]; ++k) {
    const size_t it = (size_t)ctx->pb_surv_it[k];
    if (it >= w) continue;
    if (T) std::memcpy(T + 16 * it, &ctx->pb_surv_T[16 * k], 64);
    if (inliers) inliers[it] = ctx->pb_surv_inl[k];
    if (error) error[it] = ctx->pb_surv_err[k];
  }
  *n_out = made;
  return OPE_OK;
}

}  // extern "C"
