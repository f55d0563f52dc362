// corr_sac_batch.hip — estimateCoarsePose with the correspondence aligner (feature matches, CorrespondenceRejectorSampleConsensus,
// TransformationEstimationSVD over what remains) for one model and many candidate clusters in one call (ope_corr_sac_pose_batch,
// gfx950, wave64).  DESIGN.md §4.23; the arithmetic of every step is corr_sac_math.hpp's, which ope_corr_sac runs too.
//
// The single path pays per cluster its own sampling, normals, FPFH, uploads, index build, 13 launches and 3 synchronisations of
// ope_corr_sac and 10 001 draws.  Here every stage runs once for all clusters:
//   a. the front end of ope_coarse_pose_batch (coarse_front_launch: key points, normals, FPFH of the model and every cluster);
//   b. block (model key u, active cluster a): the nearest cluster row of the model's row u (feature_knn_block, k = 1) and its distance;
//   c. one block per cluster compacts the rows that found a match into the match list, in key order, and lays the pairs out as two
//      float4 each; one block per cluster adds the nine running sums of the threshold in match order; the lists, counts and
//      thresholds come back (second synchronisation, the first is the front end's);
//   d. the host draws (cs_draw): clusters with the same seed and the same matched model rows share one list, drawn once and uploaded
//      once, three 16-bit positions per sample; a (first sample, count) record per cluster says which list to read;
//   e. one lane per (cluster, hypothesis) fits Umeyama over its three pairs;
//   f. the hot kernel: block (x, a, z) scores hypotheses [256 x, 256 x + 256) of cluster a against the tiles z, z + gridDim.z, ... of
//      its matches; the split of the matches comes from the block count of the whole batch, and with a split of one the counts are
//      stored, not added;
//   g. the counts come back (third synchronisation); the host replays RandomSampleConsensus::computeModel per cluster (cs_replay)
//      and uploads the winners' indices;
//   h. one block per cluster packs the winner's inliers (all matches without a model), the segmented pairs-sum and Umeyama launches
//      fit them; T_best, T_svd, positions and counts come back (fourth synchronisation).
// Neither the launches nor the synchronisations depend on the clusters, the hypotheses, the matches, the inliers or the iteration a
// replay stops at; nothing is summed across clusters, and a cluster's arrays sit at offsets that depend on the model alone.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "coarse_stages.hpp"
#include "corr_sac_math.hpp"
#include "stage_host.hpp"

namespace ope {
namespace {

// what the kernels of one call read and write; per active cluster a: nsk slots of the match arrays, Hmax slots of the hypotheses'
struct CbView {
  const float4 *kp;           // key points packed by segment (segment 0 = the model)
  const float *fpfh;          // 33 floats per key point
  const uint32_t *key_off;    // nseg + 1
  const int2 *active;         // na: .x = the segment of active cluster a
  int32_t *nn;                // na * nsk: the nearest cluster row of model row u, -1 without one
  float *nd;                  // ... and its squared distance
  int32_t *msrc, *mtgt;       // na * nsk: the match list (model key, cluster key), nm[a] entries
  float *mdist;
  float4 *ps, *pt;            // the matched points in match order
  uint32_t *nm;               // na
  double *thr;                // na: sample_dist_thresh
  uint32_t nsk, Hmax;
};

// b. CorrespondenceEstimation: block (u, a) = model row u among the rows of active cluster a
__global__ __launch_bounds__(256) void csb_match_kernel(CbView v) {
  const uint32_t seg = (uint32_t)v.active[blockIdx.y].x, t0 = v.key_off[seg], nt = v.key_off[seg + 1] - t0;
  const float *tf = v.fpfh + (size_t)t0 * 33, *q = v.fpfh + (size_t)(v.key_off[0] + blockIdx.x) * 33;
  const size_t u = (size_t)blockIdx.y * v.nsk + blockIdx.x;
  feature_knn_block(tf, (int)nt, q, 1, v.nn + u);
  if (threadIdx.x == 0) v.nd[u] = cs_row_dist(tf, q, v.nn[u]);
}

// c1. the match list of cluster a = blockIdx.x in key order: lane l owns the rows [kCsPackItems l, kCsPackItems l + kCsPackItems)
__global__ __launch_bounds__(1024) void csb_compact_kernel(CbView v) {
  const uint32_t a = blockIdx.x, seg = (uint32_t)v.active[a].x, t0 = v.key_off[seg], nt = v.key_off[seg + 1] - t0, s0 = v.key_off[0];
  const size_t base = (size_t)a * v.nsk;
  int32_t t[kCsPackItems];
  uint32_t mine = 0;
#pragma unroll
  for (int k = 0; k < kCsPackItems; ++k) {
    const uint32_t u = threadIdx.x * kCsPackItems + k;
    t[k] = u < v.nsk ? v.nn[base + u] : -1;
    if ((uint32_t)t[k] >= nt) t[k] = -1;   // (no finite distance: no match)
    mine += t[k] >= 0 ? 1u : 0u;
  }
  uint32_t total;
  uint32_t slot = cs_block_prefix(mine, total);
#pragma unroll
  for (int k = 0; k < kCsPackItems; ++k) {
    if (t[k] < 0) continue;
    const uint32_t u = threadIdx.x * kCsPackItems + k;
    const float4 s = v.kp[s0 + u], q = v.kp[t0 + (uint32_t)t[k]];
    v.msrc[base + slot] = (int32_t)u;
    v.mtgt[base + slot] = t[k];
    v.mdist[base + slot] = v.nd[base + u];
    v.ps[base + slot] = make_float4(s.x, s.y, s.z, 0.f);
    v.pt[base + slot] = make_float4(q.x, q.y, q.z, 0.f);
    ++slot;
  }
  if (threadIdx.x == 0) v.nm[a] = total;
}

// c2. computeSampleDistanceThreshold of cluster a = blockIdx.x (0 without a match, where the single call launches nothing)
__global__ __launch_bounds__(kCsBlock) void csb_thresh_kernel(CbView v) {
  const uint32_t a = blockIdx.x, n = v.nm[a];
  if (n == 0) {
    if (threadIdx.x == 0) v.thr[a] = 0.0;
    return;
  }
  cs_thresh_block(v.ps + (size_t)a * v.nsk, n, v.thr + a);
}

// e. computeModelCoefficients: one lane per (cluster, hypothesis); rec[a] = (first sample of its list, hypotheses)
__global__ __launch_bounds__(64) void csb_fit_kernel(CbView v, const uint2 *__restrict__ rec, const uint16_t *__restrict__ samp, uint32_t total,
                                                     float *__restrict__ T_out, float *__restrict__ rows_out) {
  const uint32_t g = blockIdx.x * 64 + threadIdx.x;
  if (g >= total) return;
  const uint32_t a = g / v.Hmax, h = g - a * v.Hmax;
  const uint2 r = rec[a];
  if (h >= r.y) return;
  const uint16_t *sa = samp + 3 * ((size_t)r.x + h);
  const float4 *ps = v.ps + (size_t)a * v.nsk, *pt = v.pt + (size_t)a * v.nsk;
  umeyama_fit(3, [&](int i, float4 &p, float4 &q) { p = ps[sa[i]]; q = pt[sa[i]]; }, T_out + 16 * (size_t)g, rows_out + 12 * (size_t)g);
}

// f. countWithinDistance of every hypothesis of every cluster: block (x, a, z) = hypotheses [256 x, 256 x + 256) of cluster a
// against the tiles z, z + gridDim.z, ... of its matches (cs_count_tiles, the single call's loop).  A lane keeps its hypothesis's
// twelve floats in registers.  Counts are integers: with the matches split over z the atomics' order does not show; without a split
// they are stored.
__global__ __launch_bounds__(kCsBlock) void csb_count_kernel(const float4 *__restrict__ ps_all, const float4 *__restrict__ pt_all,
                                                             const uint32_t *__restrict__ nm, const uint2 *__restrict__ rec,
                                                             const float *__restrict__ rows, uint32_t nsk, uint32_t Hmax, double thr2,
                                                             uint32_t *__restrict__ counts) {
  const uint32_t a = blockIdx.y, H = rec[a].y;
  if (blockIdx.x * kCsBlock >= H) return;   // (the whole block: its cluster drew fewer hypotheses)
  const uint32_t h = blockIdx.x * kCsBlock + threadIdx.x;
  const bool live = h < H;
  const size_t g = (size_t)a * Hmax + h;
  float F[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) F[i] = live ? rows[12 * g + i] : 0.f;
  const uint32_t cnt = cs_count_tiles(ps_all + (size_t)a * nsk, pt_all + (size_t)a * nsk, nm[a], F, thr2, blockIdx.z, gridDim.z);
  if (!live) return;
  if (gridDim.z == 1) counts[g] = cnt;
  else if (cnt) atomicAdd(counts + g, cnt);
}

// h1. selectWithinDistance of cluster a's winner (winner[a] < 0: no model, every match), and T_best
__global__ __launch_bounds__(1024) void csb_pack_kernel(CbView v, const int32_t *__restrict__ winner, const float *__restrict__ T,
                                                         const float *__restrict__ rows, double thr2, int32_t *__restrict__ pos,
                                                         float *__restrict__ sx, float *__restrict__ tx, uint32_t *__restrict__ pcnt,
                                                         float *__restrict__ T_best) {
  const uint32_t a = blockIdx.x;
  const int32_t w = winner[a];
  const size_t base = (size_t)a * v.nsk, g = (size_t)a * v.Hmax + (size_t)(w < 0 ? 0 : w);
  float F[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) F[i] = w >= 0 ? rows[12 * g + i] : 0.f;
  if (threadIdx.x < 16) T_best[16 * (size_t)a + threadIdx.x] = w >= 0 ? T[16 * g + threadIdx.x] : ((threadIdx.x % 5u) == 0 ? 1.f : 0.f);
  cs_pack_block(v.ps + base, v.pt + base, v.nm[a], F, thr2, w < 0 ? 1 : 0, pos + base, sx + 3 * base, tx + 3 * base, pcnt + a);
}

// the partial sums ope_rigid_transform_svd's launch would use for n pairs
__device__ __forceinline__ uint32_t csb_svd_blocks(uint32_t n) { return min(max((n + 255u) / 256u, 1u), 512u); }

// h2. block (b, a): partial b of cluster a's remaining pairs, strided and summed as pairs_sums_kernel does with its own grid
__global__ __launch_bounds__(256) void csb_pairs_sums_kernel(const float *__restrict__ sx, const float *__restrict__ tx,
                                                             const uint32_t *__restrict__ pcnt, uint32_t nsk, uint32_t max_blocks,
                                                             double *__restrict__ partials) {
  const uint32_t a = blockIdx.y, n = pcnt[a], nb = csb_svd_blocks(n);
  if (n == 0 || blockIdx.x >= nb) return;
  const size_t base = 3 * (size_t)a * nsk;
  pairs_sums_block(sx + base, tx + base, n, blockIdx.x, nb, partials + (size_t)a * kNumSums * max_blocks);
}

// h3. one wave per cluster: the partials in block order, Umeyama
__global__ __launch_bounds__(64) void csb_pairs_umeyama_kernel(const double *__restrict__ partials, const float *__restrict__ sx,
                                                               const uint32_t *__restrict__ pcnt, uint32_t nsk, uint32_t max_blocks,
                                                               float *__restrict__ T_svd) {
  const uint32_t a = blockIdx.x, n = pcnt[a];
  if (n == 0) return;
  pairs_umeyama_block(partials + (size_t)a * kNumSums * max_blocks, (int)csb_svd_blocks(n), sx + 3 * (size_t)a * nsk, T_svd + 16 * (size_t)a);
}

}  // namespace

int corr_sac_pose_batch_impl(ope_ctx *ctx, const char *who, const ope_cloud *model, size_t n, const ope_cloud *const *clusters,
                             const ope_coarse_params *front, const ope_corr_sac_params *params, const uint64_t *seeds, int keep_hypotheses,
                             ope_corr_sac_batch_result *out) {
  if (!ctx) return OPE_EINVAL;
  if (n == 0) return OPE_OK;
  if (!model || !clusters || !out) return set_err(ctx, OPE_EINVAL, std::string(who) + "bad argument");
  if (n > 65535) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than 65535 clusters (one grid row each)");
  ope_coarse_params fp;
  ope_coarse_default_params(&fp);
  if (front) fp = *front;
  ope_corr_sac_params p;
  ope_corr_sac_default_params(&p);
  if (params) p = *params;
  if (const int rc = corr_sac_check_params(ctx, who, p)) return rc;
  const size_t Hmax = (size_t)p.max_iterations + 1;
  if ((unsigned long long)n * (unsigned long long)Hmax > 0x7fffffffull)
    return set_err(ctx, OPE_EINVAL, std::string(who) + "clusters x (max_iterations + 1) above 2^31 - 1");
  if (const int rc = refuse_communicator(ctx, who)) return rc;
  // the front end's refusals (sizes, key points; the model needs three key points)
  fp.sacia.nr_samples = 3; fp.sacia.k_correspondences = 1; fp.sacia.max_iterations = p.max_iterations;
  long long model_keys = -2;
  { const int rc = coarse_batch_check(ctx, model, n, clusters, fp, &model_keys, who); if (rc != OPE_OK) return rc; }

  OPE_HIP(ctx, hipSetDevice(ctx->device));
  TraceRange r_all(ctx, "corr_sac_batch");
  ope_corr_sac_batch_stats &St = ctx->csb_stats;
  St = ope_corr_sac_batch_stats{};
  St.clusters = (int64_t)n;
  ctx->csb_match_off.clear(); ctx->csb_inl_off.clear(); ctx->csb_hyp_off.clear(); ctx->csb_list_off.clear();
  ctx->csb_msrc.clear(); ctx->csb_mtgt.clear(); ctx->csb_mdist.clear(); ctx->csb_inl_pos.clear();
  ctx->csb_counts.clear(); ctx->csb_T.clear(); ctx->csb_list_of.clear(); ctx->csb_list_samp.clear();
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
    ope_corr_sac_batch_result &o = out[i];
    std::memset(&o, 0, sizeof o);
    std::memcpy(o.T_svd, kIdentity4, sizeof kIdentity4);
    std::memcpy(o.T_best, kIdentity4, sizeof kIdentity4);
    o.best = -1;
    o.n_src_keys = (int32_t)nsk;
    o.n_tgt_keys = (int32_t)(key_off[i + 2] - key_off[i + 1]);
    o.status = clusters[i]->n == 0 ? OPE_CORRSAC_EMPTY_TARGET : o.n_tgt_keys < 10 ? OPE_CORRSAC_FEW_TARGET_FEATURES : OPE_CORRSAC_OK;
    if (o.status == OPE_CORRSAC_OK) { active.push_back(make_int2((int)(i + 1), 0)); active_cluster.push_back(i); }
  }
  const size_t na = active.size();
  St.active = (int64_t)na;
  ctx->csb_match_off.assign(n + 1, 0);
  ctx->csb_inl_off.assign(n + 1, 0);
  if (na == 0) {   // nothing reached the matcher: no launch after the front end, 2 synchronisations (key offsets, the features)
    e = coarse_front_download(ctx, fr);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    ++St.host_syncs;
    if (e != hipSuccess) return fail("download");
    coarse_front_keep(ctx, fr);
    return OPE_OK;
  }

  // ---- b, c. matches, match lists, thresholds
  TraceRange r_al(ctx, "corr_sac_batch_align");
  const size_t slots = na * (size_t)nsk, hyps = na * Hmax;
  const size_t down_bytes = 12 * na + 12 * slots;   // [thr (8 na) | nm (4 na) | msrc | mtgt | mdist]
  auto *d_active = (int2 *)tmp.get(sizeof(int2) * na, e);
  auto *d_nn = (int32_t *)tmp.get(4 * slots, e);
  auto *d_nd = (float *)tmp.get(4 * slots, e);
  auto *d_down = (unsigned char *)tmp.get(down_bytes, e);
  auto *d_ps = (float4 *)tmp.get(16 * slots, e);
  auto *d_pt = (float4 *)tmp.get(16 * slots, e);
  if (e == hipSuccess) e = upload_staged(st, d_active, active.data(), sizeof(int2) * na, &St.launches, &St.host_syncs);
  if (e != hipSuccess) return fail("buffers");
  CbView v{};
  v.kp = fr.d_kp; v.fpfh = fr.d_fpfh; v.key_off = fr.d_key_off; v.active = d_active;
  v.nn = d_nn; v.nd = d_nd;
  v.thr = (double *)d_down;
  v.nm = (uint32_t *)(d_down + 8 * na);
  v.msrc = (int32_t *)(d_down + 12 * na);
  v.mtgt = v.msrc + slots;
  v.mdist = (float *)(v.mtgt + slots);
  v.ps = d_ps; v.pt = d_pt;
  v.nsk = nsk; v.Hmax = (uint32_t)Hmax;
  STAGE_LAUNCH(ctx, St.launches, csb_match_kernel, 132.0 * (double)na * (double)nsk * (double)fr.max_keys, dim3(nsk, (unsigned)na), dim3(256), 0, st, v);
  STAGE_LAUNCH(ctx, St.launches, csb_compact_kernel, 52.0 * (double)slots, dim3((unsigned)na), dim3(1024), 0, st, v);
  STAGE_LAUNCH(ctx, St.launches, csb_thresh_kernel, 16.0 * (double)slots, dim3((unsigned)na), dim3(kCsBlock), 0, st, v);
  std::vector<unsigned char> down(down_bytes);
  e = hipGetLastError();
  if (e == hipSuccess) e = coarse_front_download(ctx, fr);
  if (e == hipSuccess) e = hipMemcpyAsync(down.data(), d_down, down_bytes, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  ++St.host_syncs;
  if (e != hipSuccess) return fail("matches");
  coarse_front_keep(ctx, fr);
  const double *h_thr = (const double *)down.data();
  const uint32_t *h_nm = (const uint32_t *)(down.data() + 8 * na);
  const int32_t *h_msrc = (const int32_t *)(down.data() + 12 * na), *h_mtgt = h_msrc + slots;
  const float *h_mdist = (const float *)(h_mtgt + slots);
  for (size_t a = 0; a < na; ++a) {
    if (h_nm[a] > nsk) return set_err(ctx, OPE_EHIP, std::string(who) + "a match list is longer than the model's key points");
    for (uint32_t j = 0; j < h_nm[a]; ++j)
      if ((uint32_t)h_msrc[a * nsk + j] >= nsk) return set_err(ctx, OPE_EHIP, std::string(who) + "a match names no model key point");
  }

  // ---- d. the draws: one list per (seed, matched model rows), three 16-bit positions per sample
  std::vector<uint64_t> seed_of(na);
  std::vector<int> list_of(na, -1);
  std::vector<std::vector<int32_t>> lists;
  std::vector<size_t> list_first;   // the cluster a list was drawn for
  {
    std::unordered_multimap<uint64_t, int> by_hash;
    std::vector<float4> src_pts;
    const float4 *model_kp = fr.h_kp.data() + key_off[0];
    for (size_t a = 0; a < na; ++a) {
      seed_of[a] = seeds ? seeds[active_cluster[a]] : p.seed;
      const uint32_t m = h_nm[a];
      if (m < 3) continue;   // no sample, no model
      const int32_t *ms = h_msrc + a * nsk;
      uint64_t hash = 1469598103934665603ull ^ seed_of[a];
      for (uint32_t j = 0; j < m; ++j) hash = (hash ^ (uint64_t)(uint32_t)ms[j]) * 1099511628211ull;
      const auto range = by_hash.equal_range(hash);
      for (auto it = range.first; it != range.second && list_of[a] < 0; ++it) {
        const size_t b = list_first[(size_t)it->second];
        if (seed_of[b] == seed_of[a] && h_nm[b] == m && std::memcmp(h_msrc + b * nsk, ms, 4 * (size_t)m) == 0) list_of[a] = it->second;
      }
      if (list_of[a] >= 0) {
        // (the same points through the same adds: anything else is a fault of this code)
        if (std::memcmp(&h_thr[a], &h_thr[list_first[(size_t)list_of[a]]], 8) != 0)
          return set_err(ctx, OPE_EHIP, std::string(who) + "clusters with the same matched model rows differ in sample_dist_thresh");
        continue;
      }
      src_pts.resize(m);
      for (uint32_t j = 0; j < m; ++j) { const float4 q = model_kp[ms[j]]; src_pts[j] = make_float4(q.x, q.y, q.z, 0.f); }
      lists.emplace_back();
      cs_draw(src_pts.data(), (int)m, h_thr[a], (uint32_t)(seed_of[a] & 0xffffffffull), Hmax, lists.back());
      list_first.push_back(a);
      list_of[a] = (int)lists.size() - 1;
      by_hash.emplace(hash, list_of[a]);
    }
  }
  St.draw_lists = (int64_t)lists.size();
  std::vector<size_t> list_off(lists.size() + 1, 0);   // in samples
  for (size_t l = 0; l < lists.size(); ++l) list_off[l + 1] = list_off[l] + lists[l].size() / 3;
  const size_t n_samp = list_off[lists.size()];
  if (n_samp > 0xffffffffull) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than 2^32 - 1 samples drawn");
  const size_t up_bytes = 8 * na + 6 * std::max<size_t>(n_samp, 1);   // [rec (8 na) | samples]
  std::vector<unsigned char> up(up_bytes, 0);
  std::vector<uint32_t> H_of(na, 0);
  {
    auto *rec = (uint2 *)up.data();
    auto *s16 = (uint16_t *)(up.data() + 8 * na);
    for (size_t l = 0; l < lists.size(); ++l)
      for (size_t j = 0; j < lists[l].size(); ++j) s16[3 * list_off[l] + j] = (uint16_t)lists[l][j];
    for (size_t a = 0; a < na; ++a) {
      if (list_of[a] >= 0) H_of[a] = (uint32_t)(list_off[(size_t)list_of[a] + 1] - list_off[(size_t)list_of[a]]);
      rec[a] = make_uint2(list_of[a] >= 0 ? (uint32_t)list_off[(size_t)list_of[a]] : 0u, H_of[a]);
      St.hypotheses += H_of[a];
    }
  }
  auto *d_up = (unsigned char *)tmp.get(up_bytes, e);
  auto *d_T = (float *)tmp.get(64 * hyps, e);
  auto *d_rows = (float *)tmp.get(48 * hyps, e);
  auto *d_cnt = (uint32_t *)tmp.get(4 * hyps, e);
  auto *d_winner = (int32_t *)tmp.get(4 * na, e);
  const size_t fin_bytes = 132 * na + 4 * slots;   // [pcnt (4 na) | T_best (64 na) | T_svd (64 na) | positions]
  auto *d_fin = (unsigned char *)tmp.get(fin_bytes, e);
  auto *d_sx = (float *)tmp.get(12 * slots, e);
  auto *d_tx = (float *)tmp.get(12 * slots, e);
  const uint32_t max_blocks = std::min<uint32_t>(std::max<uint32_t>((nsk + 255) / 256, 1), 512);
  auto *d_part = (double *)tmp.get(sizeof(double) * kNumSums * (size_t)max_blocks * na, e);
  if (e != hipSuccess) return fail("buffers");
  e = upload_staged(st, d_up, up.data(), up_bytes, &St.launches, &St.host_syncs);
  if (e == hipSuccess) e = hipMemsetAsync(d_cnt, 0, 4 * hyps, st);
  ++St.launches;
  if (e != hipSuccess) return fail("upload");
  const auto *d_rec = (const uint2 *)d_up;
  const auto *d_samp = (const uint16_t *)(d_up + 8 * na);

  // ---- e, f. fits and counts
  const double thr2 = p.inlier_threshold * p.inlier_threshold;
  STAGE_LAUNCH(ctx, St.launches, csb_fit_kernel, 208.0 * (double)St.hypotheses, dim3(grid_of(hyps, 64)), dim3(64), 0, st, v, d_rec, d_samp, (uint32_t)hyps, d_T,
               d_rows);
  uint32_t nm_max = 0;
  unsigned long long hyp_blocks = 0;
  for (size_t a = 0; a < na; ++a) {
    nm_max = std::max(nm_max, h_nm[a]);
    hyp_blocks += (H_of[a] + kCsBlock - 1) / kCsBlock;
  }
  const unsigned hb = grid_of(Hmax, kCsBlock), tiles = grid_of(nm_max, kCsTile);
  const unsigned split = (unsigned)std::min<unsigned long long>(tiles, std::max<unsigned long long>(1, (2ull * (unsigned)ctx->n_cu + hyp_blocks - 1) / std::max<unsigned long long>(hyp_blocks, 1)));
  STAGE_LAUNCH(ctx, St.launches, csb_count_kernel, 32.0 * (double)nm_max * (double)hyp_blocks + 52.0 * (double)St.hypotheses, dim3(hb, (unsigned)na, split),
               dim3(kCsBlock), 0, st, (const float4 *)d_ps, (const float4 *)d_pt, (const uint32_t *)v.nm, d_rec, (const float *)d_rows, nsk, (uint32_t)Hmax,
               thr2, d_cnt);
  std::vector<uint32_t> cnts(hyps);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(cnts.data(), d_cnt, 4 * hyps, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  ++St.host_syncs;
  if (e != hipSuccess) return fail("counts");

  // ---- g. RandomSampleConsensus::computeModel per cluster
  std::vector<int32_t> winner(na, -1);
  std::vector<uint32_t> n_rem(na, 0);
  for (size_t a = 0; a < na; ++a) {
    ope_corr_sac_batch_result &o = out[active_cluster[a]];
    o.seed = seed_of[a];
    o.sample_dist_thresh = h_thr[a];
    o.matches = (int32_t)h_nm[a];
    n_rem[a] = h_nm[a];
    if (h_nm[a] == 0) continue;
    int best = -1;
    long long best_cnt = 0;
    o.iterations = cs_replay(&cnts[a * Hmax], H_of[a], h_nm[a], p.max_iterations, p.probability, &best, &best_cnt);
    o.best = best;
    o.found = best >= 0 ? 1 : 0;
    winner[a] = best;
    if (best >= 0) n_rem[a] = (uint32_t)best_cnt;
  }
  e = upload_staged(st, d_winner, winner.data(), 4 * na, &St.launches, &St.host_syncs);
  if (e != hipSuccess) return fail("upload");

  // ---- h. the remaining matches and their pose
  auto *d_pcnt = (uint32_t *)d_fin;
  auto *d_Tbest = (float *)(d_fin + 4 * na);
  auto *d_Tsvd = (float *)(d_fin + 68 * na);
  auto *d_pos = (int32_t *)(d_fin + 132 * na);
  STAGE_LAUNCH(ctx, St.launches, csb_pack_kernel, 92.0 * (double)slots, dim3((unsigned)na), dim3(1024), 0, st, v, (const int32_t *)d_winner, (const float *)d_T,
               (const float *)d_rows, thr2, d_pos, d_sx, d_tx, d_pcnt, d_Tbest);
  STAGE_LAUNCH(ctx, St.launches, csb_pairs_sums_kernel, 24.0 * (double)slots, dim3(max_blocks, (unsigned)na), dim3(256), 0, st, (const float *)d_sx,
               (const float *)d_tx, (const uint32_t *)d_pcnt, nsk, max_blocks, d_part);
  STAGE_LAUNCH(ctx, St.launches, csb_pairs_umeyama_kernel, 136.0 * (double)max_blocks * (double)na, dim3((unsigned)na), dim3(64), 0, st, (const double *)d_part,
               (const float *)d_sx, (const uint32_t *)d_pcnt, nsk, max_blocks, d_Tsvd);
  std::vector<unsigned char> fin(fin_bytes);
  std::vector<float> Ts;
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(fin.data(), d_fin, fin_bytes, hipMemcpyDeviceToHost, st);
  if (keep_hypotheses) {
    Ts.resize(16 * hyps);
    if (e == hipSuccess) e = hipMemcpyAsync(Ts.data(), d_T, 64 * hyps, hipMemcpyDeviceToHost, st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  ++St.host_syncs;
  if (e != hipSuccess) return fail("inliers");
  const auto *h_pcnt = (const uint32_t *)fin.data();
  const auto *h_Tbest = (const float *)(fin.data() + 4 * na), *h_Tsvd = (const float *)(fin.data() + 68 * na);
  const auto *h_pos = (const int32_t *)(fin.data() + 132 * na);
  for (size_t a = 0; a < na; ++a) {
    ope_corr_sac_batch_result &o = out[active_cluster[a]];
    if (h_pcnt[a] != n_rem[a]) return set_err(ctx, OPE_EHIP, std::string(who) + "a winner's inlier list and its count disagree");
    o.inliers = (int32_t)n_rem[a];
    if (winner[a] >= 0) std::memcpy(o.T_best, h_Tbest + 16 * a, 64);
    if (n_rem[a]) std::memcpy(o.T_svd, h_Tsvd + 16 * a, 64);
  }

  // ---- what the retrieval calls hand out
  for (size_t i = 0, a = 0; i < n; ++i) {
    const bool act = a < na && active_cluster[a] == i;
    ctx->csb_match_off[i + 1] = ctx->csb_match_off[i] + (act ? h_nm[a] : 0);
    ctx->csb_inl_off[i + 1] = ctx->csb_inl_off[i] + (act ? n_rem[a] : 0);
    if (act) {
      ctx->csb_msrc.insert(ctx->csb_msrc.end(), h_msrc + a * nsk, h_msrc + a * nsk + h_nm[a]);
      ctx->csb_mtgt.insert(ctx->csb_mtgt.end(), h_mtgt + a * nsk, h_mtgt + a * nsk + h_nm[a]);
      ctx->csb_mdist.insert(ctx->csb_mdist.end(), h_mdist + a * nsk, h_mdist + a * nsk + h_nm[a]);
      ctx->csb_inl_pos.insert(ctx->csb_inl_pos.end(), h_pos + a * nsk, h_pos + a * nsk + n_rem[a]);
      ++a;
    }
  }
  if (keep_hypotheses) {
    ctx->csb_hyp_off.assign(n + 1, 0);
    ctx->csb_list_of.assign(n, -1);
    ctx->csb_list_off.assign(list_off.begin(), list_off.end());
    for (const std::vector<int32_t> &l : lists) ctx->csb_list_samp.insert(ctx->csb_list_samp.end(), l.begin(), l.end());
    for (size_t i = 0, a = 0; i < n; ++i) {
      const bool act = a < na && active_cluster[a] == i;
      ctx->csb_hyp_off[i + 1] = ctx->csb_hyp_off[i] + (act ? H_of[a] : 0);
      if (!act) continue;
      ctx->csb_list_of[i] = list_of[a];
      ctx->csb_T.insert(ctx->csb_T.end(), Ts.begin() + 16 * a * Hmax, Ts.begin() + 16 * (a * Hmax + H_of[a]));
      ctx->csb_counts.insert(ctx->csb_counts.end(), cnts.begin() + a * Hmax, cnts.begin() + a * Hmax + H_of[a]);
      ++a;
    }
  }
  return OPE_OK;
}

}  // namespace ope

using namespace ope;

extern "C" {

int ope_corr_sac_pose_batch(ope_ctx *ctx, const ope_cloud *model, size_t n, const ope_cloud *const *clusters, const ope_coarse_params *front,
                            const ope_corr_sac_params *params, const uint64_t *seeds, int keep_hypotheses, ope_corr_sac_batch_result *out) {
  return corr_sac_pose_batch_impl(ctx, "ope_corr_sac_pose_batch: ", model, n, clusters, front, params, seeds, keep_hypotheses, out);
}

int ope_corr_sac_batch_last_stats(const ope_ctx *ctx, ope_corr_sac_batch_stats *out) {
  if (!ctx || !out) return OPE_EINVAL;
  *out = ctx->csb_stats;
  return OPE_OK;
}

int ope_corr_sac_batch_matches(const ope_ctx *ctx, int which, int32_t *src_key, int32_t *tgt_key, float *dist, size_t cap, size_t *n_out) {
  if (!ctx || !n_out) return OPE_EINVAL;
  *n_out = 0;
  const std::vector<size_t> &off = ctx->csb_match_off;
  if (off.empty() || which < 0 || (size_t)which + 1 >= off.size()) return OPE_EINVAL;
  const size_t b = off[(size_t)which], made = off[(size_t)which + 1] - b, w = std::min(made, cap);
  if (src_key && w) std::memcpy(src_key, ctx->csb_msrc.data() + b, 4 * w);
  if (tgt_key && w) std::memcpy(tgt_key, ctx->csb_mtgt.data() + b, 4 * w);
  if (dist && w) std::memcpy(dist, ctx->csb_mdist.data() + b, 4 * w);
  *n_out = made;
  return OPE_OK;
}

int ope_corr_sac_batch_inliers(const ope_ctx *ctx, int which, int32_t *pos, int32_t *src_key, int32_t *tgt_key, size_t cap, size_t *n_out) {
  if (!ctx || !n_out) return OPE_EINVAL;
  *n_out = 0;
  const std::vector<size_t> &off = ctx->csb_inl_off;
  if (off.empty() || which < 0 || (size_t)which + 1 >= off.size()) return OPE_EINVAL;
  const size_t b = off[(size_t)which], made = off[(size_t)which + 1] - b, w = std::min(made, cap), m0 = ctx->csb_match_off[(size_t)which];
  for (size_t j = 0; j < w; ++j) {
    const int32_t q = ctx->csb_inl_pos[b + j];
    if (pos) pos[j] = q;
    if (src_key) src_key[j] = ctx->csb_msrc[m0 + (size_t)q];
    if (tgt_key) tgt_key[j] = ctx->csb_mtgt[m0 + (size_t)q];
  }
  *n_out = made;
  return OPE_OK;
}

int ope_corr_sac_batch_hypotheses(const ope_ctx *ctx, int which, int32_t *samples, float *T, int32_t *counts, size_t cap, size_t *n_out) {
  if (!ctx || !n_out) return OPE_EINVAL;
  *n_out = 0;
  if (ctx->csb_match_off.empty() || which < 0 || (size_t)which + 1 >= ctx->csb_match_off.size()) return OPE_EINVAL;
  const std::vector<size_t> &off = ctx->csb_hyp_off;
  if (off.empty()) return OPE_OK;   // the call did not keep them
  const size_t b = off[(size_t)which], made = off[(size_t)which + 1] - b, w = std::min(made, cap);
  const int32_t l = ctx->csb_list_of[(size_t)which];
  if (samples && w && l >= 0) std::memcpy(samples, ctx->csb_list_samp.data() + 3 * ctx->csb_list_off[(size_t)l], 12 * w);
  if (T && w) std::memcpy(T, ctx->csb_T.data() + 16 * b, 64 * w);
  if (counts && w) std::memcpy(counts, ctx->csb_counts.data() + b, 4 * w);
  *n_out = made;
  return OPE_OK;
}

}  // extern "C"
