// final_batch.hip — the reference's first-frame candidate loop (rosinterface.cpp:243-262): PoseEstimator::estimateFinalPose of
// one model against many clusters in one call (ope_final_pose_batch, gfx950, wave64).
//
// Per cluster the loop runs the coarse stage, moves the model by the coarse pose, prepares both fine clouds (NaN removal,
// UniformSampling at 8 mm, k-NN normals, NaN-normal drop: poseestimator.cpp:186-223), indexes the target and runs the fine
// ICP.  Here each step runs once for all clusters ("segments": the n moved models, then the n clusters):
//   0. the coarse stage of ope_coarse_pose_batch (coarse_pose_batch_impl), seeds counted as the estimator counts its coarse calls;
//   1. one launch moves the model n times (pcl::transformPointCloud's float operations) and takes every segment's exact bounding
//      box; one launch turns the boxes into UniformSampling's voxel geometry on the device;
//   2. the segmented uniform sampling and k-NN normals of ope_coarse_pose_batch (coarse_stages.hpp) at the fine leaf and k;
//   3. one workgroup per segment drops the rows with a non-finite normal and puts the rest in the Morton order ope_cloud_upload
//      gives a cloud (morton.hpp: 30-bit keys over the cloud's own box, a stable sort), all in LDS;
//   4. the n target trees in one pass (build_bvh_batch_device: the tree build_bvh_device builds, node for node);
//   5. the fine ICP of ope_icp_run_batch (icp_batch_core) on views of these buffers.
// Neither the launches nor the host synchronisations depend on n, and nothing is summed across clusters.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "bvh_traverse.hpp"
#include "coarse_stages.hpp"
#include "morton.hpp"
#include "stage_host.hpp"

namespace ope {

namespace {

constexpr int kFineItems = 16;   // 256 threads x 16 items: the key points of one fine cloud in one workgroup
static_assert(kCoarseBlock * kFineItems >= OPE_COARSE_MAX_KEYS, "a fine cloud must fit one workgroup");

// order-preserving integer image of a float (min / max by integer atomics)
__device__ __forceinline__ uint32_t fenc(float f) {
  const uint32_t b = (uint32_t)__float_as_int(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float fdec(uint32_t u) {
  const uint32_t b = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  return __int_as_float((int)b);
}

struct FineIn {
  CloudView c;   // the model (segments < n) or a cluster
  float T[16];   // column-major; applied to the first c.n_valid points when moved != 0
  int moved;
};

// 1a. segment s < n: the model moved by T (m0*x + m4*y + m8*z + m12, every operation rounded, in this order); s >= n: the cluster.
// Points past n_valid (non-finite) are copied as they are.  box: per segment the images of min x y z, max x y z of its finite
// points; bad |= 2 if moving made a finite point non-finite.  A wave whose lanes all hold finite points of one segment (nearly
// all of them) reduces its images first and issues one set of atomics: per-lane atomics on six words per segment took 1 ms at
// 8 clusters of C1 size.
__global__ __launch_bounds__(kCoarseBlock) void fine_transform_kernel(const FineIn *__restrict__ segs, const uint32_t *__restrict__ off,
                                                                        uint32_t nseg, uint32_t total, float4 *__restrict__ out,
                                                                        uint32_t *__restrict__ box, uint32_t *__restrict__ bad) {
  const uint32_t p = blockIdx.x * kCoarseBlock + threadIdx.x;
  const bool active = p < total;
  uint32_t s = 0xffffffffu;
  bool fin = false;
  uint32_t im[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};   // min images, max images
  if (active) {
    s = seg_of(off, nseg, p);
    const uint32_t i = p - off[s];
    const FineIn &g = segs[s];
    float4 q = g.c.xyzw[i];
    fin = i < g.c.n_valid;
    if (fin && g.moved) {
      const float *m = g.T;
      const float x = q.x, y = q.y, z = q.z;
      q.x = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], x), __fmul_rn(m[4], y)), __fmul_rn(m[8], z)), m[12]);
      q.y = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[1], x), __fmul_rn(m[5], y)), __fmul_rn(m[9], z)), m[13]);
      q.z = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[2], x), __fmul_rn(m[6], y)), __fmul_rn(m[10], z)), m[14]);
      if (!(isfinite(q.x) && isfinite(q.y) && isfinite(q.z))) atomicOr(bad, 2u);
    }
    out[p] = q;
    if (fin) { im[0] = im[3] = fenc(q.x); im[1] = im[4] = fenc(q.y); im[2] = im[5] = fenc(q.z); }
  }
  const uint32_t s0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)s);
  if (__ballot(!(fin && s == s0)) == 0ull) {
    for (int o = 32; o >= 1; o >>= 1)
      for (int d = 0; d < 3; ++d) {
        im[d] = min(im[d], (uint32_t)__shfl_xor((int)im[d], o, 64));
        im[3 + d] = max(im[3 + d], (uint32_t)__shfl_xor((int)im[3 + d], o, 64));
      }
    if ((threadIdx.x & 63u) != 0u) return;
  } else if (!fin) {
    return;
  }
  uint32_t *b = box + 6 * s;
  for (int d = 0; d < 3; ++d) { atomicMin(b + d, im[d]); atomicMax(b + 3 + d, im[3 + d]); }
}

// 1b. UniformSampling's voxel geometry of every segment from its box (ope_coarse_pose_batch's host arithmetic); bad |= 1 where PCL
// would refuse the leaf (the voxel index overflows an int)
__global__ __launch_bounds__(64) void fine_geom_kernel(CoarseSeg *__restrict__ segs, const uint32_t *__restrict__ box, uint32_t nseg,
                                                       float inv, uint32_t *__restrict__ bad) {
  const uint32_t s = blockIdx.x * 64 + threadIdx.x;
  if (s >= nseg) return;
  CoarseSeg &g = segs[s];
  long long min_b[3] = {0, 0, 0}, div_b[3] = {1, 1, 1};
  if (g.c.n_valid > 0) {
    for (int d = 0; d < 3; ++d) {
      min_b[d] = (long long)floorf(__fmul_rn(fdec(box[6 * s + d]), inv));
      div_b[d] = (long long)floorf(__fmul_rn(fdec(box[6 * s + 3 + d]), inv)) - min_b[d] + 1;
    }
    if ((double)div_b[0] * (double)div_b[1] * (double)div_b[2] >= 2147483648.0) atomicOr(bad, 1u);
  }
  for (int d = 0; d < 3; ++d) g.min_b[d] = (int)min_b[d];
  g.div_x = (uint32_t)div_b[0];
  g.div_xy = (uint32_t)(div_b[0] * div_b[1]);
  g.inv_leaf = inv;
}

// 3. one workgroup per segment: drop the key points whose normal is not finite (withNormals), then the order ope_cloud_upload gives
// the rest: Morton keys over their own bounding box, a stable sort (keys, then position).  out_xyz: {x, y, z, position before the
// sort}, out_nrm: {normal, 0}, both at the segment's first key slot; cnt / box (lo xyz, hi xyz) per segment.
__global__ __launch_bounds__(kCoarseBlock) void fine_order_kernel(const float4 *__restrict__ kp, const float4 *__restrict__ nrm,
                                                                    const uint32_t *__restrict__ key_off, float4 *__restrict__ out_xyz,
                                                                    float4 *__restrict__ out_nrm, uint32_t *__restrict__ out_cnt,
                                                                    float *__restrict__ out_box) {
  using Sort = rocprim::block_radix_sort<uint32_t, kCoarseBlock, kFineItems, uint32_t>;
  using Scan = rocprim::block_scan<uint32_t, kCoarseBlock>;
  __shared__ typename Sort::storage_type s_sort;
  __shared__ typename Scan::storage_type s_scan;
  __shared__ uint32_t s_slot[kCoarseBlock * kFineItems];   // kept position -> key slot in the segment
  __shared__ uint32_t s_box[6];
  const uint32_t s = blockIdx.x, b = key_off[s], m = key_off[s + 1] - b;
  if (threadIdx.x < 3) { s_box[threadIdx.x] = 0xffffffffu; s_box[3 + threadIdx.x] = 0u; }
  bool keep[kFineItems];
  uint32_t mine = 0;
#pragma unroll
  for (int i = 0; i < kFineItems; ++i) {   // blocked: item i of thread t is key slot t * kFineItems + i
    const uint32_t p = threadIdx.x * kFineItems + i;
    keep[i] = false;
    if (p < m) { const float4 n = nrm[b + p]; keep[i] = isfinite(n.x) && isfinite(n.y) && isfinite(n.z); }
    mine += keep[i] ? 1u : 0u;
  }
  uint32_t first = 0, total = 0;
  Scan().exclusive_scan(mine, first, 0u, total, s_scan, rocprim::plus<uint32_t>());
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kFineItems; ++i) {
    if (!keep[i]) continue;
    const uint32_t p = threadIdx.x * kFineItems + i;
    s_slot[first++] = p;
    const float4 q = kp[b + p];
    atomicMin(&s_box[0], fenc(q.x)); atomicMin(&s_box[1], fenc(q.y)); atomicMin(&s_box[2], fenc(q.z));
    atomicMax(&s_box[3], fenc(q.x)); atomicMax(&s_box[4], fenc(q.y)); atomicMax(&s_box[5], fenc(q.z));
  }
  __syncthreads();
  float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f}, iv[3] = {0.f, 0.f, 0.f};
  if (total > 0)
    for (int d = 0; d < 3; ++d) {
      lo[d] = fdec(s_box[d]);
      hi[d] = fdec(s_box[3 + d]);
      iv[d] = hi[d] > lo[d] ? __fdiv_rn(1023.999f, __fsub_rn(hi[d], lo[d])) : 0.f;
    }
  uint32_t keys[kFineItems], vals[kFineItems];
#pragma unroll
  for (int i = 0; i < kFineItems; ++i) {   // blocked over the kept positions
    const uint32_t c = threadIdx.x * kFineItems + i;
    vals[i] = c;
    keys[i] = 0xffffffffu;   // (padding sorts behind every key)
    if (c < total) {
      const float4 q = kp[b + s_slot[c]];
      keys[i] = morton_code_dev(q.x, q.y, q.z, lo[0], lo[1], lo[2], iv[0], iv[1], iv[2]);
    }
  }
  Sort().sort(keys, vals, s_sort, 0, 32);
#pragma unroll
  for (int i = 0; i < kFineItems; ++i) {
    const uint32_t q = threadIdx.x * kFineItems + i;
    if (q >= total) continue;
    const uint32_t c = vals[i], slot = s_slot[c];
    const float4 pt = kp[b + slot], n = nrm[b + slot];
    out_xyz[b + q] = make_float4(pt.x, pt.y, pt.z, __int_as_float((int)c));
    out_nrm[b + q] = make_float4(n.x, n.y, n.z, 0.f);
  }
  if (threadIdx.x == 0) {
    out_cnt[s] = total;
    for (int d = 0; d < 3; ++d) { out_box[6 * s + d] = lo[d]; out_box[6 * s + 3 + d] = hi[d]; }
  }
}

}  // namespace

// ope_final_pose_batch's refusals before anything is launched (n >= 1): parameters, and the clusters' sizes and fine key points
// (the moved models' can only be counted after sampling)
int final_batch_check(ope_ctx *ctx, size_t n, const ope_cloud *const *clusters, const ope_final_params &p) {
  static const char *who = "ope_final_pose_batch: ";
  if (!(p.fine_leaf > 0)) return set_err(ctx, OPE_EINVAL, std::string(who) + "fine_leaf must be > 0");
  if (p.fine_normals_k < 1 || p.fine_normals_k > kKnnMaxK) return set_err(ctx, OPE_EINVAL, std::string(who) + "1 <= fine_normals_k <= 32");
  { const int rc = icp_batch_check_params(ctx, p.icp); if (rc != OPE_OK) return rc; }
  // the clusters' fine key points can be counted before anything is launched (the moved models' only after sampling)
  const float inv = 1.0f / p.fine_leaf;
  for (size_t i = 0; i < n; ++i) {
    const ope_cloud *c = clusters[i];
    const std::string at = " (cluster " + std::to_string(i) + ")";
    if (!c) return set_err(ctx, OPE_EINVAL, std::string(who) + "no cluster cloud" + at);
    if (c->n > (size_t)OPE_COARSE_MAX_POINTS) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than OPE_COARSE_MAX_POINTS points" + at);
    if (c->n_valid == 0) continue;
    { const int rch = c->ensure_host(); if (rch != OPE_OK) return rch; }
    const long long kc = host_key_count(c, inv);
    if (kc < 0) return set_err(ctx, OPE_EINVAL, std::string(who) + "fine_leaf too small for the input dataset" + at);
    if (kc > OPE_COARSE_MAX_KEYS) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than OPE_COARSE_MAX_KEYS fine key points" + at);
  }

  return OPE_OK;
}

// Steps 1-4 of ope_final_pose_batch for n (model, cluster) pairs: segment i < n is the model moved by coarse[i].T when
// coarse[i].status == OPE_COARSE_OK (as it is otherwise), segment n + i cluster i.  Buffers come from tmp.
int final_fine_prepare(ope_ctx *ctx, CallTmp &tmp, const char *who, const ope_cloud *model, size_t n, const ope_cloud *const *clusters,
                       const ope_final_params &p, const ope_coarse_batch_result *coarse, FinePrep &out) {
  const float inv = 1.0f / p.fine_leaf;
  std::vector<uint32_t> &key_off = out.key_off, &cnt = out.cnt;
  std::vector<float> &fbox = out.fbox;
  std::vector<int32_t> &status = out.status;
  std::vector<size_t> &icp_of = out.icp_of;
  std::vector<BvhBatchTree> &trees = out.trees;
  uint32_t &nkeys = out.nkeys;
  float4 *&d_fxyz = out.d_fxyz, *&d_fnrm = out.d_fnrm;
  const size_t nseg = 2 * n;
  std::vector<FineIn> fin(nseg);
  std::vector<CoarseSeg> segs(nseg);
  std::vector<uint32_t> off(nseg + 1, 0);
  for (size_t s = 0; s < nseg; ++s) {
    const bool src = s < n;
    const ope_cloud *c = src ? model : clusters[s - n];
    fin[s].c = c->view();
    fin[s].moved = src && coarse[s].status == OPE_COARSE_OK;
    std::memcpy(fin[s].T, fin[s].moved ? coarse[s].T : kIdentity4, sizeof kIdentity4);
    off[s + 1] = off[s] + (uint32_t)c->n;
  }
  const uint32_t total = off[nseg];

  hipError_t e = hipSuccess;
  auto fail = [&](const char *what) { return set_err(ctx, OPE_EHIP, std::string(who) + what + ": " + hipGetErrorString(e)); };
  auto *d_fin = (FineIn *)tmp.get(sizeof(FineIn) * nseg, e);
  auto *d_segs = (CoarseSeg *)tmp.get(sizeof(CoarseSeg) * nseg, e);
  auto *d_off = (uint32_t *)tmp.get(4 * (nseg + 1), e);
  auto *d_raw = (float4 *)tmp.get(16 * (size_t)std::max<uint32_t>(total, 1), e);
  auto *d_box = (uint32_t *)tmp.get(4 * (6 * nseg + 1), e);   // 6 images per segment, then the `bad` word
  if (e != hipSuccess) return fail("buffers");
  uint32_t *d_bad = d_box + 6 * nseg;
  // the sampled segments are the moved copies / the clusters in d_raw (finite points first, w = original index)
  for (size_t s = 0; s < nseg; ++s) {
    segs[s].c = CloudView{d_raw + off[s], nullptr, off[s + 1] - off[s], fin[s].c.n_valid};
    std::memset(segs[s].min_b, 0, sizeof segs[s].min_b);
    segs[s].div_x = segs[s].div_xy = 1;
    segs[s].inv_leaf = inv;
  }
  e = h2d_copy(ctx->stream, d_fin, fin.data(), sizeof(FineIn) * nseg);
  if (e == hipSuccess) e = h2d_copy(ctx->stream, d_segs, segs.data(), sizeof(CoarseSeg) * nseg);
  if (e == hipSuccess) e = h2d_copy(ctx->stream, d_off, off.data(), 4 * (nseg + 1));
  {
    // empty boxes: the min images above every image, the max images (and `bad`) below
    std::vector<uint32_t> init(6 * nseg + 1, 0u);
    for (size_t s = 0; s < nseg; ++s) init[6 * s] = init[6 * s + 1] = init[6 * s + 2] = 0xffffffffu;
    if (e == hipSuccess) e = h2d_copy(ctx->stream, d_box, init.data(), 4 * init.size());
  }
  if (e != hipSuccess) return fail("buffers");

  // ---- 1. move, bound, voxel geometry
  {
    TraceRange r(ctx, "final_transform");
    {
      KernelTimer kt(ctx, "fine_transform_kernel", 32.0 * total);
      if (total)
        hipLaunchKernelGGL(fine_transform_kernel, dim3((total + kCoarseBlock - 1) / kCoarseBlock), dim3(kCoarseBlock), 0, ctx->stream, d_fin, d_off,
                           (uint32_t)nseg, total, d_raw, d_box, d_bad);
    }
    STAGE_LAUNCH_TIMED(ctx, fine_geom_kernel, "fine_geom_kernel", 0.0, dim3((unsigned)((nseg + 63) / 64)), dim3(64), 0, ctx->stream, d_segs, d_box,
                       (uint32_t)nseg, inv, d_bad);
    e = hipGetLastError();
    if (e != hipSuccess) return fail("transform");
  }

  // ---- 2. uniform sampling (one synchronisation: the key counts), refusals, normals
  float4 *d_kp = nullptr;
  uint32_t *d_key_off = nullptr;
  uint32_t bad = 0;   // (comes back with the key offsets)
  {
    const char *what = "";
    e = coarse_sample_segments(ctx, tmp, d_segs, d_off, nseg, total, &d_kp, &d_key_off, key_off, what, d_bad, &bad, 4);
    if (e != hipSuccess) return fail(what);
  }
  if (bad & 2u) return set_err(ctx, OPE_EINVAL, std::string(who) + "a coarse pose moves a finite model point out of float range");
  if (bad & 1u) return set_err(ctx, OPE_EINVAL, std::string(who) + "fine_leaf too small for a moved model");
  nkeys = key_off[nseg];
  uint32_t max_keys = 0;
  for (size_t s = 0; s < nseg; ++s) {
    const uint32_t m = key_off[s + 1] - key_off[s];
    if (m > (uint32_t)OPE_COARSE_MAX_KEYS)
      return set_err(ctx, OPE_EINVAL, std::string(who) + "more than OPE_COARSE_MAX_KEYS fine key points (" +
                                          (s < n ? "the model moved for cluster " + std::to_string(s) : "cluster " + std::to_string(s - n)) + ")");
    max_keys = std::max(max_keys, m);
  }
  std::vector<int2> tiles;
  for (size_t s = 0; s < nseg; ++s)
    for (uint32_t q = 0; q < key_off[s + 1] - key_off[s]; q += kCoarseBlock) tiles.push_back(make_int2((int)s, (int)q));
  const size_t nk1 = std::max<size_t>(nkeys, 1);
  auto *d_tiles = (int2 *)tmp.get(sizeof(int2) * std::max<size_t>(tiles.size(), 1), e);
  auto *d_nrm = (float4 *)tmp.get(16 * nk1, e);
  d_fxyz = (float4 *)tmp.get(16 * nk1, e);
  d_fnrm = (float4 *)tmp.get(16 * nk1, e);
  auto *d_cnt = (uint32_t *)tmp.get(4 * nseg + 4 * 6 * nseg, e);
  if (e == hipSuccess && !tiles.empty()) e = h2d_copy(ctx->stream, d_tiles, tiles.data(), sizeof(int2) * tiles.size());
  if (e != hipSuccess) return fail("buffers");
  float *d_fbox = reinterpret_cast<float *>(d_cnt + nseg);
  {
    TraceRange r(ctx, "final_normals");
    e = coarse_normals_launch(ctx, d_kp, d_key_off, d_tiles, tiles.size(), nkeys, max_keys, p.fine_normals_k, p.coarse.viewpoint, d_nrm);
    if (e != hipSuccess) return fail("normals");
  }

  // ---- 3. NaN-normal drop and the upload order; one synchronisation: the fine clouds' sizes and boxes
  STAGE_LAUNCH_TIMED(ctx, fine_order_kernel, "fine_order_kernel", 64.0 * nkeys, dim3((unsigned)nseg), dim3(kCoarseBlock), 0, ctx->stream, d_kp, d_nrm,
                     d_key_off, d_fxyz, d_fnrm, d_cnt, d_fbox);
  cnt.assign(nseg, 0u);
  fbox.assign(6 * nseg, 0.f);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(cnt.data(), d_cnt, 4 * nseg, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(fbox.data(), d_fbox, 4 * 6 * nseg, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return fail("fine clouds");

  // ---- 4. the target trees of every cluster that runs ICP
  status.assign(n, 0);
  icp_of.clear();
  for (size_t i = 0; i < n; ++i) {
    const uint32_t nt = cnt[n + i];
    if (clusters[i]->n == 0) status[i] = OPE_FINAL_EMPTY_TARGET;
    else if ((long long)nt < (long long)std::max(p.min_fine_points, 1)) status[i] = OPE_FINAL_FEW_FINE_POINTS;
    else status[i] = coarse[i].status == OPE_COARSE_OK ? OPE_FINAL_OK : OPE_FINAL_FEW_TARGET_FEATURES;
    if (status[i] == OPE_FINAL_OK || status[i] == OPE_FINAL_FEW_TARGET_FEATURES) icp_of.push_back(i);
  }
  const size_t np = icp_of.size();
  if (np) {
    ope_index_params ip;
    ope_index_default_params(&ip);
    trees.assign(np, BvhBatchTree{});
    std::vector<size_t> node_off(np), pts_off(np);
    size_t nodes_total = 0, pts_total = 0;
    int max_depth = bvh_depth(OPE_COARSE_MAX_KEYS, ip.leaf_size);   // the fit launches of any batch: those of the deepest tree allowed
    for (size_t a = 0; a < np; ++a) {
      const size_t s = n + icp_of[a];
      BvhBatchTree &t = trees[a];
      t.n = cnt[s];
      t.D = bvh_depth(t.n, ip.leaf_size);
      t.scale = bvh_scale(&fbox[6 * s], &fbox[6 * s + 3]);
      node_off[a] = nodes_total;
      pts_off[a] = pts_total;
      nodes_total += (size_t)2 << t.D;
      pts_total += t.n + kPtsPad;
      max_depth = std::max(max_depth, t.D);
    }
    auto *d_nodes = (float4 *)tmp.get(48 * nodes_total, e);
    auto *d_axis2 = (float4 *)tmp.get(16 * nodes_total, e);
    auto *d_tpts = (float4 *)tmp.get(16 * pts_total, e);
    auto *d_tnrm = (float4 *)tmp.get(16 * pts_total, e);
    auto *d_trees = (BvhBatchTree *)tmp.get(sizeof(BvhBatchTree) * np, e);
    if (e != hipSuccess) return fail("buffers");
    for (size_t a = 0; a < np; ++a) {
      const size_t s = n + icp_of[a];
      BvhBatchTree &t = trees[a];
      t.src = d_fxyz + key_off[s];
      t.src_nrm = d_fnrm + key_off[s];
      t.nodes = d_nodes + 3 * node_off[a];
      t.axis2 = d_axis2 + node_off[a];
      t.pts = d_tpts + pts_off[a];
      t.nrm = d_tnrm + pts_off[a];
    }
    e = hipMemsetAsync(d_tpts, 0, 16 * pts_total, ctx->stream);   // (the kPtsPad entries past every tree's points)
    if (e == hipSuccess) e = h2d_copy(ctx->stream, d_trees, trees.data(), sizeof(BvhBatchTree) * np);
    if (e == hipSuccess) {
      TraceRange r(ctx, "final_index_build");
      e = build_bvh_batch_device(ctx, d_trees, np, max_depth);
    }
    if (e != hipSuccess) return fail("index build");

  }
  return OPE_OK;
}

}  // namespace ope

using namespace ope;

extern "C" {

void ope_final_default_params(ope_final_params *p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  ope_coarse_default_params(&p->coarse);
  p->fine_leaf = 0.008f;
  p->fine_normals_k = 30;
  p->min_fine_points = 100;
  ope_icp_default_params(&p->icp);
  p->icp.max_iterations = 100;
  p->icp.transformation_epsilon = 1e-8;
  p->icp.euclidean_fitness_epsilon = 1e-8;
  p->icp.corr_mode = OPE_CORR_NORMAL_SHOOTING;
  p->icp.k_normal_shooting = 20;
  p->icp.use_surface_normal_rej = 1;
  p->icp.surface_normal_thr = 0.7;
  p->fitness_max_range = DBL_MAX;
  p->accept_fitness = 1e-4;
  p->accept_strength = 0.4;
}

int ope_final_pose_batch(ope_ctx *ctx, const ope_cloud *model, size_t n, const ope_cloud *const *clusters, const ope_final_params *params,
                         const uint64_t *seeds, ope_final_batch_result *out, int32_t *selected) {
  static const char *who = "ope_final_pose_batch: ";
  if (!ctx) return set_err(ctx, OPE_EINVAL, "ope_final_pose_batch: bad argument");
  if (selected) *selected = -1;
  ctx->final_off.clear();   // (ope_final_batch_inputs reports "no call yet" unless this call succeeds)
  if (n == 0) return OPE_OK;
  if (!model || !clusters || !out) return set_err(ctx, OPE_EINVAL, std::string(who) + "bad argument");
  if (n > 65535) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than 65535 clusters (one grid row each)");
  ope_final_params p;
  ope_final_default_params(&p);
  if (params) p = *params;
  { const int rc = final_batch_check(ctx, n, clusters, p); if (rc != OPE_OK) return rc; }

  // ---- 0. the coarse stage (its own refusals come before it launches anything)
  std::vector<ope_coarse_batch_result> coarse(n);
  std::vector<uint64_t> seed_used(n, 0);
  {
    const int rc = coarse_pose_batch_impl(ctx, model, n, clusters, &p.coarse, seeds, seeds == nullptr, coarse.data(), seed_used.data());
    if (rc != OPE_OK) return rc;
  }
  return final_batch_finish(ctx, who, model, n, clusters, p, coarse.data(), seed_used.data(), out, selected);
}

int ope_final_pose_batch_rejectors(ope_ctx *ctx, const ope_cloud *model, size_t n, const ope_cloud *const *clusters, const ope_final_params *params,
                                   const ope_global_rejector *list, size_t n_list, const uint64_t *seeds, ope_final_batch_result *out,
                                   int32_t *selected) {
  static const char *who = "ope_final_pose_batch_rejectors: ";
  if (!ctx) return set_err(ctx, OPE_EINVAL, "ope_final_pose_batch_rejectors: bad argument");
  if (n_list == 0) return ope_final_pose_batch(ctx, model, n, clusters, params, seeds, out, selected);   // no list: that call
  if (selected) *selected = -1;
  ctx->final_off.clear();
  ope_final_params p;
  ope_final_default_params(&p);
  if (params) p = *params;
  { const int rc = icp_batch_check_list(ctx, "ope_final_pose_batch_rejectors", p.icp, list, n_list); if (rc != OPE_OK) return rc; }
  if (n == 0) return OPE_OK;
  if (!model || !clusters || !out) return set_err(ctx, OPE_EINVAL, std::string(who) + "bad argument");
  if (n > 65535) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than 65535 clusters (one grid row each)");
  { const int rc = final_batch_check(ctx, n, clusters, p); if (rc != OPE_OK) return rc; }

  // ---- 0. the coarse stage of ope_final_pose_batch
  std::vector<ope_coarse_batch_result> coarse(n);
  std::vector<uint64_t> seed_used(n, 0);
  {
    const int rc = coarse_pose_batch_impl(ctx, model, n, clusters, &p.coarse, seeds, seeds == nullptr, coarse.data(), seed_used.data());
    if (rc != OPE_OK) return rc;
  }
  return final_batch_finish(ctx, who, model, n, clusters, p, coarse.data(), seed_used.data(), out, selected, list, n_list);
}

}  // extern "C"

int ope::final_batch_finish(ope_ctx *ctx, const char *who, const ope_cloud *model, size_t n, const ope_cloud *const *clusters,
                            const ope_final_params &p, const ope_coarse_batch_result *coarse, const uint64_t *seed_used,
                            ope_final_batch_result *out, int32_t *selected, const ope_global_rejector *list, size_t n_list) {
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  TraceRange r_all(ctx, "final_batch");
  const size_t nseg = 2 * n;
  CallTmp tmp{ctx->stream, {}};
  FinePrep fp;
  { const int rc = final_fine_prepare(ctx, tmp, who, model, n, clusters, p, coarse, fp); if (rc != OPE_OK) return rc; }
  const std::vector<uint32_t> &key_off = fp.key_off, &cnt = fp.cnt;
  const std::vector<float> &fbox = fp.fbox;
  const std::vector<int32_t> &status = fp.status;
  const std::vector<size_t> &icp_of = fp.icp_of;
  const std::vector<BvhBatchTree> &trees = fp.trees;
  const uint32_t nkeys = fp.nkeys;
  float4 *const d_fxyz = fp.d_fxyz, *const d_fnrm = fp.d_fnrm;
  hipError_t e = hipSuccess;
  auto fail = [&](const char *what) { return set_err(ctx, OPE_EHIP, std::string(who) + what + ": " + hipGetErrorString(e)); };
  const size_t np = icp_of.size();
  std::vector<ope_icp_batch_result> icp_out(std::max<size_t>(np, 1));
  if (np) {
    // ---- 5. the fine ICP: ope_icp_run_batch on clouds and indexes that view these buffers
    std::vector<ope_cloud> src_v(np);
    std::vector<ope_index> tgt_v(np);
    std::vector<const ope_cloud *> src_p(np);
    std::vector<const ope_index *> tgt_p(np);
    for (size_t a = 0; a < np; ++a) {
      const size_t i = icp_of[a], ss = i, st = n + i;
      ope_cloud &c = src_v[a];
      c.ctx = ctx;
      c.n = c.n_valid = cnt[ss];
      c.d_xyzw = d_fxyz + key_off[ss];
      c.d_nrm = d_fnrm + key_off[ss];
      std::memcpy(c.bb_lo, &fbox[6 * ss], 12);
      std::memcpy(c.bb_hi, &fbox[6 * ss + 3], 12);
      ope_index &x = tgt_v[a];
      x.ctx = ctx;
      x.n = x.n_total = cnt[st];
      x.depth = trees[a].D;
      x.d_nodes = trees[a].nodes;
      x.d_pts = trees[a].pts;
      x.d_nrm = trees[a].nrm;
      x.d_axis2 = trees[a].axis2;
      std::memcpy(x.bb_lo, &fbox[6 * st], 12);
      std::memcpy(x.bb_hi, &fbox[6 * st + 3], 12);
      for (int d = 0; d < 3; ++d) x.pivot[d] = 0.5 * ((double)x.bb_lo[d] + (double)x.bb_hi[d]);
      src_p[a] = &c;
      tgt_p[a] = &x;
    }
    TraceRange r(ctx, "final_icp");
    const BatchStageReq req{list, n_list, nullptr, nullptr, nullptr};
    const int rc = icp_batch_core(ctx, np, src_p.data(), tgt_p.data(), nullptr, p.icp, p.fitness_max_range, icp_out.data(), n_list > 0 ? &req : nullptr);
    if (rc != OPE_OK) return rc;
  }

  // ---- the fine inputs, kept for ope_final_batch_inputs (key-point order: w is the position before the upload order)
  std::vector<float4> hx(nkeys), hn(nkeys);
  if (nkeys) e = hipMemcpyAsync(hx.data(), d_fxyz, 16 * (size_t)nkeys, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && nkeys) e = hipMemcpyAsync(hn.data(), d_fnrm, 16 * (size_t)nkeys, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return fail("download");
  ctx->final_off.assign(nseg + 1, 0);
  for (size_t w = 0; w < nseg; ++w) {   // cloud 2i = source of cluster i (segment i), 2i + 1 = its target (segment n + i)
    const size_t s = (w & 1) ? n + w / 2 : w / 2;
    ctx->final_off[w + 1] = ctx->final_off[w] + cnt[s];
  }
  ctx->final_xyz.assign(3 * (size_t)ctx->final_off[nseg], 0.f);
  ctx->final_nrm.assign(3 * (size_t)ctx->final_off[nseg], 0.f);
  for (size_t w = 0; w < nseg; ++w) {
    const size_t s = (w & 1) ? n + w / 2 : w / 2;
    for (uint32_t q = 0; q < cnt[s]; ++q) {
      const float4 a = hx[key_off[s] + q], b = hn[key_off[s] + q];
      int32_t c;
      std::memcpy(&c, &a.w, 4);
      float *x = &ctx->final_xyz[3 * ((size_t)ctx->final_off[w] + (size_t)c)], *m = &ctx->final_nrm[3 * ((size_t)ctx->final_off[w] + (size_t)c)];
      x[0] = a.x; x[1] = a.y; x[2] = a.z;
      m[0] = b.x; m[1] = b.y; m[2] = b.z;
    }
  }

  // ---- results
  size_t a = 0;
  for (size_t i = 0; i < n; ++i) {
    ope_final_batch_result &o = out[i];
    std::memset(&o, 0, sizeof o);
    o.coarse = coarse[i];
    o.seed = seed_used[i];
    std::memcpy(o.fine.T, kIdentity4, sizeof kIdentity4);
    o.fine.fitness = std::numeric_limits<double>::max();
    o.n_fine_src = (int32_t)cnt[i];
    o.n_fine_tgt = (int32_t)cnt[n + i];
    o.status = status[i];
    if (a < np && icp_of[a] == i) {
      o.fine = icp_out[a++];
      o.accepted = (o.fine.fitness < p.accept_fitness || o.fine.result.align_strength > p.accept_strength) ? 1 : 0;
      if (o.accepted && selected && *selected < 0) *selected = (int32_t)i;
    }
  }
  return OPE_OK;
}

extern "C" {

int ope_final_pose_batch_prerejective(ope_ctx *ctx, const ope_cloud *model, size_t n, const ope_cloud *const *clusters,
                                      const ope_final_params *params, const ope_prerejective_params *prerejective, const uint64_t *seeds,
                                      ope_final_batch_result *out, int32_t *selected) {
  static const char *who = "ope_final_pose_batch_prerejective: ";
  if (!ctx) return set_err(ctx, OPE_EINVAL, "ope_final_pose_batch_prerejective: bad argument");
  if (selected) *selected = -1;
  ctx->final_off.clear();
  if (n == 0) return OPE_OK;
  if (!model || !clusters || !out) return set_err(ctx, OPE_EINVAL, std::string(who) + "bad argument");
  if (n > 65535) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than 65535 clusters (one grid row each)");
  ope_final_params p;
  ope_final_default_params(&p);
  if (params) p = *params;
  { const int rc = final_batch_check(ctx, n, clusters, p); if (rc != OPE_OK) return rc; }

  // ---- 0. the coarse stage: the prerejective aligner, seeds counted as the estimator counts its coarse calls
  std::vector<ope_prerejective_batch_result> pre(n);
  {
    const int rc = prerejective_pose_batch_impl(ctx, who, model, n, clusters, &p.coarse, prerejective, seeds, seeds == nullptr, 0, pre.data());
    if (rc != OPE_OK) return rc;
  }
  std::vector<ope_coarse_batch_result> coarse(n);
  std::vector<uint64_t> seed_used(n, 0);
  for (size_t i = 0; i < n; ++i) {
    ope_coarse_batch_result &c = coarse[i];
    std::memcpy(c.T, pre[i].T, sizeof c.T);   // (the identity without a winner: an identity pose and a counted coarse call)
    c.best_error = pre[i].error;
    c.best_iteration = pre[i].best_iteration;
    c.n_src_keys = pre[i].n_src_keys;
    c.n_tgt_keys = pre[i].n_tgt_keys;
    c.status = pre[i].status == OPE_PREREJ_OK ? OPE_COARSE_OK
               : pre[i].status == OPE_PREREJ_EMPTY_TARGET ? OPE_COARSE_EMPTY_TARGET : OPE_COARSE_FEW_TARGET_FEATURES;
    seed_used[i] = pre[i].seed;
  }
  return final_batch_finish(ctx, who, model, n, clusters, p, coarse.data(), seed_used.data(), out, selected);
}

int ope_final_pose_batch_correspondences(ope_ctx *ctx, const ope_cloud *model, size_t n, const ope_cloud *const *clusters,
                                         const ope_final_params *params, const ope_corr_sac_params *corr_sac, const uint64_t *seeds,
                                         ope_final_batch_result *out, int32_t *selected) {
  static const char *who = "ope_final_pose_batch_correspondences: ";
  if (!ctx) return set_err(ctx, OPE_EINVAL, "ope_final_pose_batch_correspondences: bad argument");
  if (selected) *selected = -1;
  ctx->final_off.clear();
  if (n == 0) return OPE_OK;
  if (!model || !clusters || !out) return set_err(ctx, OPE_EINVAL, std::string(who) + "bad argument");
  if (n > 65535) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than 65535 clusters (one grid row each)");
  ope_final_params p;
  ope_final_default_params(&p);
  if (params) p = *params;
  { const int rc = final_batch_check(ctx, n, clusters, p); if (rc != OPE_OK) return rc; }

  // ---- 0. the coarse stage: the correspondence aligner; every rejector of the reference's loop draws from the same seed
  std::vector<ope_corr_sac_batch_result> cs(n);
  {
    const int rc = corr_sac_pose_batch_impl(ctx, who, model, n, clusters, &p.coarse, corr_sac, seeds, 0, cs.data());
    if (rc != OPE_OK) return rc;
  }
  std::vector<ope_coarse_batch_result> coarse(n);
  std::vector<uint64_t> seed_used(n, 0);
  for (size_t i = 0; i < n; ++i) {
    ope_coarse_batch_result &c = coarse[i];
    std::memcpy(c.T, cs[i].T_svd, sizeof c.T);   // (the identity without a match: an identity pose and a counted coarse call)
    c.best_error = 0.0;                          // (the pipeline has no error metric)
    c.best_iteration = cs[i].best;
    c.n_src_keys = cs[i].n_src_keys;
    c.n_tgt_keys = cs[i].n_tgt_keys;
    c.status = cs[i].status == OPE_CORRSAC_OK ? OPE_COARSE_OK
               : cs[i].status == OPE_CORRSAC_EMPTY_TARGET ? OPE_COARSE_EMPTY_TARGET : OPE_COARSE_FEW_TARGET_FEATURES;
    seed_used[i] = cs[i].seed;
  }
  return final_batch_finish(ctx, who, model, n, clusters, p, coarse.data(), seed_used.data(), out, selected);
}

int ope_final_batch_inputs(ope_ctx *ctx, int which, int side, float *xyz, float *normals, size_t cap, size_t *n_out) {
  if (!ctx || !n_out || (side != 0 && side != 1)) return set_err(ctx, OPE_EINVAL, "ope_final_batch_inputs: bad argument");
  *n_out = 0;
  const std::vector<uint32_t> &off = ctx->final_off;
  if (off.empty()) return set_err(ctx, OPE_EINVAL, "ope_final_batch_inputs: no successful ope_final_pose_batch call yet");
  const long long w = 2ll * which + side;
  if (which < 0 || w + 1 >= (long long)off.size()) return set_err(ctx, OPE_EINVAL, "ope_final_batch_inputs: `which` out of range");
  const size_t b = off[w], m = off[w + 1] - b, k = std::min(m, cap);
  if (xyz) std::memcpy(xyz, ctx->final_xyz.data() + 3 * b, 12 * k);
  if (normals) std::memcpy(normals, ctx->final_nrm.data() + 3 * b, 12 * k);
  *n_out = m;
  return OPE_OK;
}

}  // extern "C"
