// track.hip — the reference's later frames (rosinterface.cpp:264-313, gfx950, wave64): the centroid gate and the gated
// estimateFinalPose of the previously aligned model in one call.
//
// The gate (ope_track_gate) runs three launches whatever the number of clusters:
//   1. one launch restores every cloud's ORIGINAL order (uploaded clouds are stored along the Morton curve, w = original index);
//   2. one workgroup per cloud takes pcl::compute3DCentroid: coalesced tiles staged in LDS, lanes 0-2 each add one coordinate in
//      the cloud's own order (a sequential float sum cannot be split), lane 3 counts; the source skips non-finite points (the
//      !is_dense branch), a cluster sums every point (is_dense);
//   3. one workgroup takes every distance (float, Eigen's order) and makes the decision the reference's loop makes.
// ope_track_pose reads that decision back once and then runs the gated cluster through the coarse stage of
// ope_coarse_pose_batch (only while the previous fine fit scored > 1e-4), the fine preparation of ope_final_pose_batch, the
// single-problem ICP (ope_icp_run on views of the prepared buffers), getFitnessScore, and the re-anchoring SVD fit from the
// original-order copies step 1 made.  The aligned model stays on the device as a new cloud.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "coarse_stages.hpp"
#include "stage_host.hpp"

namespace ope {

namespace {

constexpr int kGateBlock = 256;

struct GateSeg {
  CloudView c;
  uint32_t skip_nonfinite;   // 1: the !is_dense branch (the source)
};

// 1. cloud s's point p goes to its original position: xyz[3 * (off[s] + w)]
__global__ __launch_bounds__(kGateBlock) void track_scatter_kernel(const GateSeg *__restrict__ segs, const uint32_t *__restrict__ off, uint32_t nseg,
                                                                  uint32_t total, float *__restrict__ xyz) {
  const uint32_t p = blockIdx.x * kGateBlock + threadIdx.x;
  if (p >= total) return;
  const uint32_t s = seg_of(off, nseg, p), n = off[s + 1] - off[s];
  const float4 q = segs[s].c.xyzw[p - off[s]];
  const uint32_t o = (uint32_t)__float_as_int(q.w);
  if (o >= n) return;   // (not a cloud's index: never for a cloud ope_cloud_upload made)
  float *d = xyz + 3 * ((size_t)off[s] + o);
  d[0] = q.x; d[1] = q.y; d[2] = q.z;
}

// 2. one workgroup per cloud: centroid {x, y, z, count (int bits)}.  Lane d < 3 adds coordinate d of every counted point in
// original order, lane 3 counts; the empty cloud keeps the zero centroid (Eigen::Vector4f::Zero()).
__global__ __launch_bounds__(kGateBlock) void track_centroid_kernel(const GateSeg *__restrict__ segs, const uint32_t *__restrict__ off,
                                                                   const float *__restrict__ xyz, float4 *__restrict__ cent) {
  __shared__ float s_v[3][kGateBlock];
  __shared__ uint32_t s_ok[kGateBlock];
  const uint32_t s = blockIdx.x, b = off[s], n = off[s + 1] - b, t = threadIdx.x;
  const bool skip = segs[s].skip_nonfinite != 0;
  float acc = 0.f;
  uint32_t cnt = 0;
  for (uint32_t base = 0; base < n; base += kGateBlock) {
    const uint32_t m = min((uint32_t)kGateBlock, n - base);
    if (t < m) {
      const float *q = xyz + 3 * ((size_t)b + base + t);
      const float x = q[0], y = q[1], z = q[2];
      s_v[0][t] = x; s_v[1][t] = y; s_v[2][t] = z;
      s_ok[t] = (!skip || (isfinite(x) && isfinite(y) && isfinite(z))) ? 1u : 0u;
    }
    __syncthreads();
    if (t < 3) {
      for (uint32_t j = 0; j < m; ++j)
        if (s_ok[j]) acc = __fadd_rn(acc, s_v[t][j]);
    } else if (t == 3) {
      for (uint32_t j = 0; j < m; ++j) cnt += s_ok[j];
    }
    __syncthreads();
  }
  __shared__ float s_sum[3];
  __shared__ uint32_t s_cnt;
  if (t < 3) s_sum[t] = acc;
  if (t == 3) s_cnt = cnt;
  __syncthreads();
  if (t == 0) {
    const uint32_t c = s_cnt;
    float4 r = make_float4(0.f, 0.f, 0.f, __int_as_float((int)c));
    if (c > 0) {   // centroid /= static_cast<Scalar>(count)
      const float fc = (float)c;
      r.x = __fdiv_rn(s_sum[0], fc); r.y = __fdiv_rn(s_sum[1], fc); r.z = __fdiv_rn(s_sum[2], fc);
    }
    cent[s] = r;
  }
}

// 3. distances of clouds 1..n to cloud 0 ((dx^2 + dy^2) + dz^2, a correctly rounded sqrt), then the reference's loop:
//   distance = 10; for i: distance = d_i; if (distance < gate) { if (!empty_i) { gated = i; break; } }
//   after it: no gated cluster and distance > gate -> re-align all; otherwise nothing.
// dec = {branch, selected}
__global__ __launch_bounds__(kGateBlock) void track_decide_kernel(const float4 *__restrict__ cent, uint32_t n, double gate, float *__restrict__ dist,
                                                                 int32_t *__restrict__ dec) {
  const float4 c0 = cent[0];
  for (uint32_t i = threadIdx.x; i < n; i += kGateBlock) {
    const float4 c = cent[1 + i];
    const float dx = __fsub_rn(c.x, c0.x), dy = __fsub_rn(c.y, c0.y), dz = __fsub_rn(c.z, c0.z);
    const float sq = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    dist[i] = (float)__builtin_sqrt((double)sq);   // (a double sqrt rounded to float is the correctly rounded float sqrt)
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double distance = 10.0;
  int32_t sel = -1;
  for (uint32_t i = 0; i < n; ++i) {
    const float d = dist[i];
    distance = (double)d;
    if (distance < gate && __float_as_int(cent[1 + i].w) > 0) { sel = (int32_t)i; break; }
  }
  dec[0] = sel >= 0 ? OPE_TRACK_GATED : (distance > gate ? OPE_TRACK_REALIGN_ALL : OPE_TRACK_NOTHING);
  dec[1] = sel;
}

// The gate of n >= 1 clusters.  With model != NULL the model's original-order copy is made too (one more segment of launch 1),
// for the re-anchoring fit.  *d_xyz: original-order xyz, segment s at 3 * off[s] (s = 0 the source, 1..n the clusters, n + 1 the
// model); off receives the offsets.
int gate_run(ope_ctx *ctx, CallTmp &tmp, const ope_cloud *source, size_t n, const ope_cloud *const *clusters, const ope_cloud *model,
             double gate, ope_track_gate_result *out, ope_track_centroid *centroids, float **d_xyz, std::vector<uint32_t> &off) {
  const size_t ncent = n + 1, nseg = ncent + (model ? 1 : 0);
  std::vector<GateSeg> segs(nseg);
  off.assign(nseg + 1, 0);
  for (size_t s = 0; s < nseg; ++s) {
    const ope_cloud *c = s == 0 ? source : s <= n ? clusters[s - 1] : model;
    segs[s].c = c->view();
    segs[s].skip_nonfinite = s == 0 ? 1u : 0u;
    if ((uint64_t)off[s] + c->n > 0x7fffffffull) return set_err(ctx, OPE_EINVAL, "ope_track_gate: more than 2^31-1 points in all");
    off[s + 1] = off[s] + (uint32_t)c->n;
  }
  const uint32_t total = off[nseg];
  hipError_t e = hipSuccess;
  auto *d_segs = (GateSeg *)tmp.get(sizeof(GateSeg) * nseg, e);
  auto *d_off = (uint32_t *)tmp.get(4 * (nseg + 1), e);
  auto *d_pts = (float *)tmp.get(12 * (size_t)std::max<uint32_t>(total, 1), e);
  // read back in one copy: centroids (ncent float4), distances (n floats), the decision (2 ints)
  const size_t back_bytes = 16 * ncent + 4 * n + 8;
  auto *d_back = (unsigned char *)tmp.get(back_bytes, e);
  if (e == hipSuccess) e = h2d_copy(ctx->stream, d_segs, segs.data(), sizeof(GateSeg) * nseg);
  if (e == hipSuccess) e = h2d_copy(ctx->stream, d_off, off.data(), 4 * (nseg + 1));
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string("ope_track_gate: buffers: ") + hipGetErrorString(e));
  auto *d_cent = (float4 *)d_back;
  auto *d_dist = (float *)(d_back + 16 * ncent);
  auto *d_dec = (int32_t *)(d_back + 16 * ncent + 4 * n);
  {
    TraceRange r(ctx, "track_gate");
    {
      KernelTimer kt(ctx, "track_scatter_kernel", 28.0 * total);
      if (total)
        hipLaunchKernelGGL(track_scatter_kernel, dim3((total + kGateBlock - 1) / kGateBlock), dim3(kGateBlock), 0, ctx->stream, d_segs, d_off,
                           (uint32_t)nseg, total, d_pts);
    }
    STAGE_LAUNCH_TIMED(ctx, track_centroid_kernel, "track_centroid_kernel", 12.0 * (off[ncent]), dim3((unsigned)ncent), dim3(kGateBlock), 0, ctx->stream,
                       d_segs, d_off, d_pts, d_cent);
    STAGE_LAUNCH_TIMED(ctx, track_decide_kernel, "track_decide_kernel", 0.0, dim3(1), dim3(kGateBlock), 0, ctx->stream, d_cent, (uint32_t)n, gate, d_dist,
                       d_dec);
  }
  std::vector<unsigned char> back(back_bytes);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(back.data(), d_back, back_bytes, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string("ope_track_gate: ") + hipGetErrorString(e));
  auto cent_of = [&](size_t s, ope_track_centroid &c) {
    float v[4];
    std::memcpy(v, back.data() + 16 * s, 16);
    std::memcpy(c.centroid, v, 12);
    std::memcpy(&c.count, &v[3], 4);
    c.distance = 0.f;
    if (s > 0) std::memcpy(&c.distance, back.data() + 16 * ncent + 4 * (s - 1), 4);
  };
  cent_of(0, out->source);
  if (centroids)
    for (size_t i = 0; i < n; ++i) cent_of(i + 1, centroids[i]);
  std::memcpy(&out->branch, back.data() + 16 * ncent + 4 * n, 4);
  std::memcpy(&out->selected, back.data() + 16 * ncent + 4 * n + 4, 4);
  if (d_xyz) *d_xyz = d_pts;
  return OPE_OK;
}

int gate_checks(ope_ctx *ctx, const char *who, const ope_cloud *source, size_t n, const ope_cloud *const *clusters, ope_track_gate_result *out) {
  if (!source || (n && !clusters) || !out) return set_err(ctx, OPE_EINVAL, std::string(who) + "bad argument");
  if (n > 65535) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than 65535 clusters");
  for (size_t i = 0; i < n; ++i)
    if (!clusters[i]) return set_err(ctx, OPE_EINVAL, std::string(who) + "no cluster cloud (cluster " + std::to_string(i) + ")");
  return OPE_OK;
}

// Matrix4f::operator* of the façade (column-major, float, k in order)
void matmul4(const float *a, const float *b, float *out) {
  float r[16];
  for (int c = 0; c < 4; ++c)
    for (int row = 0; row < 4; ++row) {
      float s = 0.f;
      for (int k = 0; k < 4; ++k) s += a[4 * k + row] * b[4 * c + k];
      r[4 * c + row] = s;
    }
  std::memcpy(out, r, sizeof r);
}

}  // namespace

}  // namespace ope

using namespace ope;

extern "C" {

void ope_track_default_params(ope_track_params *p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->gate_distance = 0.05;
  p->coarse_fitness = 1e-4;
  ope_final_default_params(&p->final);
}

int ope_track_gate(ope_ctx *ctx, const ope_cloud *source, size_t n, const ope_cloud *const *clusters, const ope_track_params *params,
                   ope_track_gate_result *out, ope_track_centroid *centroids) {
  static const char *who = "ope_track_gate: ";
  if (!ctx) return set_err(ctx, OPE_EINVAL, "ope_track_gate: bad argument");
  { const int rc = gate_checks(ctx, who, source, n, clusters, out); if (rc != OPE_OK) return rc; }
  ope_track_params p;
  ope_track_default_params(&p);
  if (params) p = *params;
  std::memset(out, 0, sizeof *out);
  out->branch = OPE_TRACK_NO_CLUSTERS;
  out->selected = -1;
  if (n == 0) return OPE_OK;   // (rosinterface.cpp:220: nothing runs, not even the source's centroid)
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  CallTmp tmp{ctx->stream, {}};
  std::vector<uint32_t> off;
  return gate_run(ctx, tmp, source, n, clusters, nullptr, p.gate_distance, out, centroids, nullptr, off);
}

int ope_track_pose(ope_ctx *ctx, const ope_cloud *model, const ope_cloud *source, double fitness_fine, int64_t coarse_calls, size_t n,
                   const ope_cloud *const *clusters, const ope_track_params *params, ope_track_result *out, ope_track_centroid *centroids,
                   ope_final_batch_result *realign, ope_cloud **aligned) {
  static const char *who = "ope_track_pose: ";
  if (!ctx) return set_err(ctx, OPE_EINVAL, "ope_track_pose: bad argument");
  if (aligned) *aligned = nullptr;
  if (!model || !out || !aligned || (n && !realign)) return set_err(ctx, OPE_EINVAL, std::string(who) + "bad argument");
  { const int rc = gate_checks(ctx, who, source, n, clusters, &out->gate); if (rc != OPE_OK) return rc; }
  ope_track_params p;
  ope_track_default_params(&p);
  if (params) p = *params;
  std::memset(out, 0, sizeof *out);
  out->gate.branch = OPE_TRACK_NO_CLUSTERS;
  out->gate.selected = out->selected = -1;
  out->coarse_status = OPE_TRACK_COARSE_SKIPPED;
  out->status = OPE_FINAL_EMPTY_TARGET;
  out->fitness = std::numeric_limits<double>::max();
  for (float *m : {out->coarse, out->fine, out->rigid, out->final_pose}) std::memcpy(m, kIdentity4, sizeof kIdentity4);
  if (n == 0) return OPE_OK;
  // refusals before anything is launched: what ope_final_pose_batch refuses for (model, clusters) and, when the coarse stage is
  // to run, what the coarse stage refuses for (source, clusters)
  const bool coarse_runs = fitness_fine > p.coarse_fitness;
  if (model->n > (size_t)OPE_COARSE_MAX_POINTS || source->n > (size_t)OPE_COARSE_MAX_POINTS)
    return set_err(ctx, OPE_EINVAL, std::string(who) + "a model of more than OPE_COARSE_MAX_POINTS points");
  { const int rc = final_batch_check(ctx, n, clusters, p.final); if (rc != OPE_OK) return rc; }
  if (coarse_runs) {
    const int rc = coarse_batch_check(ctx, model, n, clusters, p.final.coarse, nullptr);
    if (rc != OPE_OK) return rc;
    const int rcs = coarse_batch_check(ctx, source, n, clusters, p.final.coarse, nullptr);
    if (rcs != OPE_OK) return rcs;
  }

  OPE_HIP(ctx, hipSetDevice(ctx->device));
  TraceRange r_all(ctx, "track_pose");
  CallTmp tmp{ctx->stream, {}};
  std::vector<uint32_t> off;
  float *d_orig = nullptr;
  { const int rc = gate_run(ctx, tmp, source, n, clusters, model, p.gate_distance, &out->gate, centroids, &d_orig, off); if (rc != OPE_OK) return rc; }
  const int branch = out->gate.branch;
  if (branch == OPE_TRACK_NOTHING) return OPE_OK;
  if (branch == OPE_TRACK_REALIGN_ALL) {
    if (!coarse_runs) { out->gate.branch = OPE_TRACK_REALIGN_LOOP; return OPE_OK; }   // (estimateFinalPoseCandidates' loop case)
    ope_final_params pf = p.final;
    pf.coarse.sacia.seed += (uint64_t)coarse_calls;   // the k-th SAC-IA call of the estimator draws with seed + k
    int32_t sel = -1;
    const int rc = ope_final_pose_batch(ctx, model, n, clusters, &pf, nullptr, realign, &sel);
    out->selected = sel;
    return rc;
  }

  // ---- GATED: estimateFinalPose(source, cluster) (poseestimator.cpp:383-448)
  const size_t g = (size_t)out->gate.selected;
  out->selected = (int32_t)g;
  const ope_cloud *cl = clusters[g];
  ope_coarse_batch_result cres;
  std::memset(&cres, 0, sizeof cres);
  std::memcpy(cres.T, kIdentity4, sizeof kIdentity4);
  cres.status = OPE_TRACK_COARSE_SKIPPED;
  cres.best_iteration = -1;
  if (coarse_runs) {
    const uint64_t seed = p.final.coarse.sacia.seed + (uint64_t)coarse_calls;
    const int rc = coarse_pose_batch_impl(ctx, source, 1, &cl, &p.final.coarse, &seed, false, &cres, nullptr);
    if (rc != OPE_OK) return rc;
    if (cres.status == OPE_COARSE_OK) out->seed = seed;
  }
  out->coarse_status = cres.status;
  std::memcpy(out->coarse, cres.T, sizeof cres.T);
  FinePrep fp;
  { const int rc = final_fine_prepare(ctx, tmp, who, source, 1, &cl, p.final, &cres, fp); if (rc != OPE_OK) return rc; }
  out->n_fine_src = (int32_t)fp.cnt[0];
  out->n_fine_tgt = (int32_t)fp.cnt[1];
  int32_t st = fp.status[0];
  if (!coarse_runs && st == OPE_FINAL_FEW_TARGET_FEATURES) st = OPE_FINAL_OK;   // (no coarse stage, not a failed one)
  out->status = st;
  if (!fp.icp_of.empty()) {
    // the single-problem ICP (ope_icp_run: many workgroups) on views of the prepared buffers
    ope_cloud c;
    c.ctx = ctx;
    c.n = c.n_valid = fp.cnt[0];
    c.d_xyzw = fp.d_fxyz + fp.key_off[0];
    c.d_nrm = fp.d_fnrm + fp.key_off[0];
    c.host_valid = false;
    std::memcpy(c.bb_lo, &fp.fbox[0], 12);
    std::memcpy(c.bb_hi, &fp.fbox[3], 12);
    ope_index x;
    x.ctx = ctx;
    x.n = x.n_total = fp.cnt[1];
    x.depth = fp.trees[0].D;
    x.d_nodes = fp.trees[0].nodes;
    x.d_pts = fp.trees[0].pts;
    x.d_nrm = fp.trees[0].nrm;
    x.d_axis2 = fp.trees[0].axis2;
    x.grid_mode = 0;
    std::memcpy(x.bb_lo, &fp.fbox[6], 12);
    std::memcpy(x.bb_hi, &fp.fbox[9], 12);
    for (int d = 0; d < 3; ++d) x.pivot[d] = 0.5 * ((double)x.bb_lo[d] + (double)x.bb_hi[d]);
    int rc;
    {
      TraceRange r(ctx, "track_icp");
      rc = ope_icp_run(ctx, &c, &x, nullptr, &p.final.icp, out->fine, &out->icp);
      if (rc == OPE_OK) rc = ope_fitness(ctx, &c, &x, out->fine, p.final.fitness_max_range, &out->fitness, nullptr, &out->fitness_n);
    }
    // the views die here: the context must not keep them as its last run
    ctx->run_src = nullptr;
    ctx->run_tgt = nullptr;
    ctx->run_active = false;
    if (rc != OPE_OK) return rc;
  }

  // ---- rigidmodelPose: the SVD fit of the model to the entry source over identity pairs (:425-436), from step 1's copies
  if (model->n > 0 && source->n >= model->n) {
    const size_t nm = model->n;
    const int nblocks = (int)std::min<size_t>((nm + 255) / 256, 512);
    hipError_t e = hipSuccess;
    auto *d_part = (double *)tmp.get(sizeof(double) * kNumSums * nblocks, e);
    auto *d_T = (float *)tmp.get(64, e);
    if (e == hipSuccess) {
      TraceRange r(ctx, "track_rigid");
      launch_pairs_svd(ctx->stream, d_orig + 3 * (size_t)off[n + 1], d_orig + 3 * (size_t)off[0], (uint32_t)nm, d_part, nblocks, d_T);
      e = hipMemcpyAsync(out->rigid, d_T, 64, hipMemcpyDeviceToHost, ctx->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + "rigid fit: " + hipGetErrorString(e));
  }
  float pose[16];
  matmul4(out->coarse, out->fine, pose);          // pose = coarsePose * finePose (:421)
  matmul4(out->rigid, pose, out->final_pose);     // finalPose = rigidmodelPose * pose (:439)

  // ---- the new aligned model, left on the device: the source moved by the coarse pose (:66-70), then by the fine pose (:358-360)
  ope_cloud empty;
  empty.ctx = ctx;
  ope_cloud *moved = nullptr;
  const ope_cloud *from = source;
  if (cres.status == OPE_COARSE_OK) {
    const int rc = ope_cloud_concat(ctx, source, out->coarse, &empty, &moved);
    if (rc != OPE_OK) return rc;
    from = moved;
  }
  const int rc = ope_cloud_concat(ctx, from, out->fine, &empty, aligned);
  if (moved) ope_cloud_free(moved);
  return rc;
}

}  // extern "C"
