// coarse_stages.hpp — the segmented stages of ope_coarse_pose_batch (coarse_batch.hip) that the batched final pose
// (final_batch.hip) runs again on its fine clouds: uniform sampling of many clouds ("segments") in one pass and k-NN normals of
// every segment's key points.  The kernels live in coarse_batch.hip; these are their host-side launchers.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "ope_internal.hpp"

namespace ope {

constexpr int kCoarseBlock = 256;

// one segment of a segmented stage: its points (finite ones first, w = original index) and its voxel geometry at inv_leaf
// (min_b / div as UniformSampling derives them from the cloud's bounding box)
struct CoarseSeg {
  CloudView c;
  int min_b[3];
  uint32_t div_x, div_xy;
  float inv_leaf;
};

// the segment that holds point p of the packed points (off: nseg + 1 starts)
__device__ __forceinline__ uint32_t seg_of(const uint32_t *__restrict__ off, uint32_t nseg, uint32_t p) {
  uint32_t lo = 0, hi = nseg;   // last segment whose start is <= p
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (off[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

// every device buffer of one call; freed on every way out
struct CallTmp {
  hipStream_t st;
  std::vector<void *> ps;
  void *get(size_t bytes, hipError_t &e) {
    void *q = nullptr;
    if (e == hipSuccess) e = tmp_malloc(st, &q, bytes);
    if (q) ps.push_back(q);
    return q;
  }
  ~CallTmp() { for (void *q : ps) tmp_free(st, q); }
};

// clusters.hip: the kw written clusters of a segmentation (host offsets `off`, device offsets d_roff, packed ORIGINAL indices d_idx
// into `cloud`) as new device clouds, each what ope_cloud_select builds, in batched launches and one synchronisation (both are
// added to *launches / *host_syncs).  d_pts_by_o / d_pos_by_o: the cloud's points and sorted positions by original index.
int clusters_build_clouds(ope_ctx *ctx, CallTmp &tmp, const char *who, const ope_cloud *cloud, size_t kw, const std::vector<uint32_t> &off,
                          const int32_t *d_idx, const uint32_t *d_roff, const float4 *d_pts_by_o, const uint32_t *d_pos_by_o,
                          ope_cloud **out_clouds, int64_t *launches, int64_t *host_syncs);

// Uniform sampling of nseg segments (d_segs, d_off: nseg + 1 point offsets, total points): one segmented radix sort, PCL's
// survivor rule per voxel run, one scan.  *d_kp (total + 1 float4): the key points packed by segment (w = original index);
// *d_key_off (nseg + 1): first slot of every segment.  key_off receives *d_key_off on the host: the call's one
// synchronisation (work enqueued before it on the stream is complete too); extra_bytes from d_extra (the caller's) come back to
// h_extra in the same synchronisation.  On failure, `what` names the step.
hipError_t coarse_sample_segments(ope_ctx *ctx, CallTmp &tmp, const CoarseSeg *d_segs, const uint32_t *d_off, size_t nseg, uint32_t total,
                                  float4 **d_kp, uint32_t **d_key_off, std::vector<uint32_t> &key_off, const char *&what,
                                  const void *d_extra = nullptr, void *h_extra = nullptr, size_t extra_bytes = 0);
// NormalEstimation (k-NN, self included, viewpoint vp) of every key point against its own segment: one workgroup per tile
// (segment, first query) of d_tiles; nkeys = all key points, max_keys = the most of one segment (the LDS it stages).
hipError_t coarse_normals_launch(ope_ctx *ctx, const float4 *d_kp, const uint32_t *d_key_off, const int2 *d_tiles, size_t n_tiles,
                                 uint32_t nkeys, uint32_t max_keys, int k, const float vp[3], float4 *d_nrm);
// distinct voxels of a cloud's finite points at 1 / inv (= its uniform-sampling key points), counted on the host with the
// device's arithmetic; -1 if PCL would refuse the leaf (the voxel index overflows an int)
long long host_key_count(const ope_cloud *c, float inv);
// ope_coarse_pose_batch.  seed_by_rank: without seeds, cluster i draws with sacia.seed + (clusters before i that reached SAC-IA)
// instead of sacia.seed + i.  seeds_used (optional, n): the seed each cluster drew with, 0 for those that did not.
int coarse_pose_batch_impl(ope_ctx *ctx, const ope_cloud *model, size_t n, const ope_cloud *const *clusters, const ope_coarse_params *params,
                           const uint64_t *seeds, bool seed_by_rank, ope_coarse_batch_result *out, uint64_t *seeds_used);

// coarse_pose_batch_impl's refusals, before anything is launched (n >= 1); *model_keys = the model's key points (optional)
// who: the entry point its errors name
int coarse_batch_check(ope_ctx *ctx, const ope_cloud *model, size_t n, const ope_cloud *const *clusters, const ope_coarse_params &p,
                       long long *model_keys, const char *who = "ope_coarse_pose_batch: ");

// The front end of the batched coarse stages (steps 1-3 of ope_coarse_pose_batch: segmented uniform sampling, normals, SPFH / FPFH)
// for the model (segment 0) and n clusters (segments 1..n), shared by ope_coarse_pose_batch and ope_prerejective_pose_batch.
// coarse_front_launch enqueues the launches (one synchronisation: the key offsets, in key_off when it returns); the device arrays
// are packed by segment from d_key_off.  coarse_front_download enqueues the copies of the key points, normals and FPFH rows to the
// host; after the caller's next synchronisation coarse_front_keep stores them for ope_coarse_batch_features.
struct CoarseFront {
  std::vector<uint32_t> key_off;   // nseg + 1
  uint32_t nkeys = 0, max_keys = 0, nsk = 0;   // all key points, the most of one segment, the model's
  float4 *d_kp = nullptr, *d_nrm = nullptr;    // w of a key point = its original index
  uint32_t *d_key_off = nullptr;
  float *d_fpfh = nullptr;                     // 33 floats per key point
  std::vector<float4> h_kp;
  std::vector<float> h_nrm4, h_fpfh;
};
int coarse_front_launch(ope_ctx *ctx, CallTmp &tmp, const char *who, const ope_cloud *model, size_t n, const ope_cloud *const *clusters,
                        const ope_coarse_params &p, long long model_keys, CoarseFront &f);
hipError_t coarse_front_download(ope_ctx *ctx, CoarseFront &f);
void coarse_front_keep(ope_ctx *ctx, CoarseFront &f);

// prerejective_batch.hip: ope_prerejective_pose_batch.  seed_by_rank as coarse_pose_batch_impl's; who: the entry point its errors name
int prerejective_pose_batch_impl(ope_ctx *ctx, const char *who, const ope_cloud *model, size_t n, const ope_cloud *const *clusters,
                                 const ope_coarse_params *front, const ope_prerejective_params *params, const uint64_t *seeds,
                                 bool seed_by_rank, int keep_hypotheses, ope_prerejective_batch_result *out);

// prerejective_draws.hip: the draws of n problems (common ns, S, K, H; host seeds) written packed (sample | pick << 12) to d_draws
// (n * H * S) by one seed upload and three launches on the context's stream; plan.fits is the caller's to check.  *d_words
// (n, from tmp): per problem kDrawOverflow / kDrawShort once the stream has run, for the caller to fetch with its next download.
struct DrawPlan;
hipError_t draws_device_launch(ope_ctx *ctx, CallTmp &tmp, const DrawPlan &plan, int ns, int S, int K, int H, const uint64_t *seeds, size_t n,
                               uint16_t *d_draws, uint32_t **d_words, int64_t *launches, int64_t *host_syncs);

// corr_sac_batch.hip: ope_corr_sac_pose_batch; who: the entry point its errors name
int corr_sac_pose_batch_impl(ope_ctx *ctx, const char *who, const ope_cloud *model, size_t n, const ope_cloud *const *clusters,
                             const ope_coarse_params *front, const ope_corr_sac_params *params, const uint64_t *seeds, int keep_hypotheses,
                             ope_corr_sac_batch_result *out);

// final_batch.hip: ope_final_pose_batch's refusals before anything is launched, and its fine preparation (steps 1-4: move,
// sample, normals, NaN-normal drop and upload order, target trees) of n (model, cluster) pairs.  Segment s < n is the model moved
// by coarse[s].T when coarse[s].status == OPE_COARSE_OK (as it is otherwise), segment n + i cluster i; per segment its fine
// points at d_fxyz / d_fnrm + key_off[s] (cnt[s] of them, box fbox[6s..6s+5]); status[i] = OPE_FINAL_*, icp_of = the clusters
// that run a fine ICP, trees[a] the target tree of icp_of[a].  who: the entry point its errors name.
struct FinePrep {
  std::vector<uint32_t> key_off, cnt;
  std::vector<float> fbox;
  std::vector<int32_t> status;
  std::vector<size_t> icp_of;
  std::vector<BvhBatchTree> trees;
  uint32_t nkeys = 0;
  float4 *d_fxyz = nullptr, *d_fnrm = nullptr;
};
int final_batch_check(ope_ctx *ctx, size_t n, const ope_cloud *const *clusters, const ope_final_params &p);
// everything of ope_final_pose_batch after its coarse stage (final_fine_prepare, icp_batch_core, the kept inputs, the results):
// coarse[i] / seed_used[i] are what out[i].coarse / .seed report; list (n_list > 0): the global rejectors of the fine ICP
// (ope_final_pose_batch_rejectors)
int final_batch_finish(ope_ctx *ctx, const char *who, const ope_cloud *model, size_t n, const ope_cloud *const *clusters, const ope_final_params &p,
                       const ope_coarse_batch_result *coarse, const uint64_t *seed_used, ope_final_batch_result *out, int32_t *selected,
                       const ope_global_rejector *list = nullptr, size_t n_list = 0);
int final_fine_prepare(ope_ctx *ctx, CallTmp &tmp, const char *who, const ope_cloud *model, size_t n, const ope_cloud *const *clusters,
                       const ope_final_params &p, const ope_coarse_batch_result *coarse, FinePrep &out);

}  // namespace ope
