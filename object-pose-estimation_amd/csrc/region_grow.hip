// region_grow.hip — smoothness-constrained region growing on the device (ope_region_grow, gfx950, wave64): what pcl::RegionGrowing
// over normals returns (SegmentationRegionGrow::getSegmentRegGrow, segmentationregiongrow.cpp:9-82) with the curvature test off,
// restated as a fixed point that runs in any order.  DESIGN.md §4.17 has the restatement and its proof.
//
//   u -> v  iff  v is one of u's number_of_neighbours nearest points (u included) and !(fabsf(n_v . n_u) < c)
//   label(v) = the smallest rank (curvature ascending, then index; NaN last) among all u that reach v, v included
//
//   1. rank: one radix sort of (curvature, original index) over the finite points.  From here on a point IS its rank.  The same
//      launch counts the points whose curvature exceeds the threshold: a non-zero count refuses the call (one small read-back);
//   2. graph: one lane per point walks the cloud's own tree from the point's own leaf (features.hip: self_leaves) for its k nearest
//      and keeps the neighbours that pass the edge test;
//   3. an edge with its reverse (mutual) puts both ends in one strongly connected component: a union-find over the mutual edges,
//      the larger root hooked to the smaller, so that a component's root is its smallest rank; the other edges are "one-way";
//   4. sweeps: per one-way edge u -> v, L[root(v)] = min(L[root(v)], L[root(u)]), and per root r a pointer jump
//      L[r] = min(L[r], L[root(L[r])]) (L[r] reaches r, so whatever reaches L[r] reaches r): a chain of h hops closes in about
//      log2(h) sweeps.  Sweeps go out four at a time; the host reads their change counters and stops after a sweep that changed
//      nothing.  No fixed number of sweeps ends the labelling;
//   5. region sizes by label, the size filter, regions by the rank of their seed (a scan over the ranks), and the points of the
//      written regions by a stable sort of the ORIGINAL indices: the conventions of ope_euclidean_clusters.
// Kernel launches booked: 19 + 5 per batch of four sweeps (+ 1 with normals passed in, + 4 for the _cloud form); host
// synchronisations: 2 + 1 per batch (+ the staged upload of passed normals, + 1 for the _cloud form).  The build of the cloud's
// tree and, when the call estimates the normals, ope_normals (its own tree, one synchronisation) are not booked.  Neither count
// depends on the number of regions.  The normals and the graph take a walk each (k = 30, k = 15): the one-walk form, which keeps
// the first 15 of the 30 nearest, is not built.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "bvh_traverse.hpp"
#include "coarse_stages.hpp"
#include "region_common.hpp"
#include "stage_host.hpp"

namespace ope {

namespace {

// normals passed in (ORIGINAL order, w = curvature) -> the cloud's sorted order
__global__ __launch_bounds__(kRgBlock) void rg_gather_normals_kernel(CloudView c, const float4 *__restrict__ nrm_by_o, float4 *__restrict__ nrm) {
  const uint32_t p = blockIdx.x * kRgBlock + threadIdx.x;
  if (p >= c.n) return;
  nrm[p] = nrm_by_o[(uint32_t)__float_as_int(c.xyzw[p].w)];
}

// 1a. sort key of a finite point: (curvature as an ordered word, original index); a NaN curvature after every finite one and
// after +inf, -0 as +0 (std::sort's `<` holds them equal: the index decides).  refused: points with curvature > threshold.
__global__ __launch_bounds__(kRgBlock) void rg_key_kernel(CloudView c, const float4 *__restrict__ nrm, float curv_thr, unsigned long long *__restrict__ keys,
                                                          uint32_t *__restrict__ vals, uint32_t *__restrict__ refused) {
  const uint32_t p = blockIdx.x * kRgBlock + threadIdx.x;
  bool over = false;
  if (p < c.n_valid) {
    float cv = nrm[p].w;
    over = cv > curv_thr;
    uint32_t w = 0xffffffffu;
    if (cv == cv) {
      uint32_t u = (uint32_t)__float_as_int(cv);
      if ((u & 0x7fffffffu) == 0u) u = 0u;
      w = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    keys[p] = ((unsigned long long)w << 32) | (uint32_t)__float_as_int(c.xyzw[p].w);
    vals[p] = p;
  }
  const unsigned long long m = __ballot(over);
  if (m && (threadIdx.x & 63u) == 0) atomicAdd(refused, (uint32_t)__popcll(m));
}

// 1b. rank of every sorted position; a point's own parent and label
__global__ __launch_bounds__(kRgBlock) void rg_rank_kernel(const uint32_t *__restrict__ sval, uint32_t n_valid, uint32_t *__restrict__ rank_of_pos,
                                                           uint32_t *__restrict__ parent, uint32_t *__restrict__ L) {
  const uint32_t r = blockIdx.x * kRgBlock + threadIdx.x;
  if (r >= n_valid) return;
  rank_of_pos[sval[r]] = r;
  parent[r] = r;
  L[r] = r;
}

// PCL's dot product: (x*x' + y*y') + z*z' in float, no contraction
__device__ __forceinline__ float dot_pcl(const float4 &a, const float4 &b) {
  return __fadd_rn(__fadd_rn(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y)), __fmul_rn(a.z, b.z));
}

// 2. one lane per finite point u: its k nearest (itself included) and, of those, the v != u with !(fabsf(n_v . n_u) < c), as sorted
// positions in adj[pos(u) * k ..]; kNone elsewhere.  (Rows by position, not by rank: the rows step 3 reads for a point are its
// neighbours', close by in the Morton order.)  KREG: the list in registers for the reference's k (15), 0: in LDS (any k <= 32).
template <int KREG>
__global__ __launch_bounds__(kKnnBlock) void rg_graph_kernel(CloudView q, BvhView tgt, const float4 *__restrict__ nrm, const uint32_t *__restrict__ pos_by_o,
                                                             const uint32_t *__restrict__ self_leaf, int k, float c, uint32_t *__restrict__ adj) {
  extern __shared__ unsigned char s_dyn[];
  float *ld = reinterpret_cast<float *>(s_dyn) + threadIdx.x;
  uint32_t *lp = reinterpret_cast<uint32_t *>(s_dyn + sizeof(float) * kKnnBlock * kKnnMaxK) + threadIdx.x;
  __shared__ float s_stk[kMaxDepth + 1][kKnnBlock];
  float *stk = &s_stk[0][threadIdx.x];
  const uint32_t lane_id = threadIdx.x & 63u;
  for (uint32_t base = blockIdx.x * kKnnBlock + (threadIdx.x & ~63u); base < q.n_valid; base += gridDim.x * kKnnBlock) {
    const uint32_t i = base + lane_id;
    const bool active = i < q.n_valid;
    const float4 s = q.xyzw[active ? i : 0];
    const uint32_t h = active ? self_leaf[(uint32_t)__float_as_int(s.w)] : 0u;
    const float4 nu = nrm[active ? i : 0];
    uint32_t *row = adj + (size_t)(active ? i : 0u) * (size_t)k;
    if constexpr (KREG > 0) {
      KnnRegVisitor<KREG> v;
      v.init(active);
      if (active) bvh_traverse(tgt, s.x, s.y, s.z, v, stk, kKnnBlock, h);
      if (active) {
#pragma unroll
        for (int j = 0; j < KREG; ++j) {
          uint32_t out = kNone;
          if (j < v.count) {
            const uint32_t pv = pos_by_o[(uint32_t)__float_as_int(tgt.pts[v.p[j]].w)];
            if (pv != i && !(fabsf(dot_pcl(nrm[pv], nu)) < c)) out = pv;
          }
          row[j] = out;
        }
      }
    } else {
      KnnVisitor v{ld, lp, kKnnBlock, k, 0, active ? INFINITY : -INFINITY};
      if (active) bvh_traverse(tgt, s.x, s.y, s.z, v, stk, kKnnBlock, h);
      if (active) {
        for (int j = 0; j < k; ++j) {
          uint32_t out = kNone;
          if (j < v.count) {
            const uint32_t pv = pos_by_o[(uint32_t)__float_as_int(tgt.pts[lp[j * kKnnBlock]].w)];
            if (pv != i && !(fabsf(dot_pcl(nrm[pv], nu)) < c)) out = pv;
          }
          row[j] = out;
        }
      }
    }
  }
}

// 3. per point u (a sorted position) and edge u -> v: mutual (u is in v's row) -> one union of the two ranks, made from the smaller
// end; otherwise the edge is kept in ow (one-way, v as its rank) and counted
__global__ __launch_bounds__(kRgBlock) void rg_mutual_kernel(const uint32_t *__restrict__ adj, const uint32_t *__restrict__ rank_of_pos, uint32_t n_valid,
                                                             int k, uint32_t *__restrict__ parent, uint32_t *__restrict__ ow,
                                                             unsigned long long *__restrict__ n_one_way) {
  const uint32_t u = blockIdx.x * kRgBlock + threadIdx.x;
  uint32_t mine = 0;
  if (u < n_valid) {
    for (int j = 0; j < k; ++j) {
      const uint32_t v = adj[(size_t)u * k + j];
      uint32_t keep = kNone;
      if (v != kNone) {
        bool mutual = false;
        for (int t = 0; t < k; ++t) mutual |= adj[(size_t)v * k + t] == u;
        if (mutual) { if (u < v) uf_union(parent, rank_of_pos[u], rank_of_pos[v]); }
        else { keep = rank_of_pos[v]; ++mine; }
      }
      ow[(size_t)u * k + j] = keep;
    }
  }
  for (int off = 32; off >= 1; off >>= 1) mine += (uint32_t)__shfl_xor((int)mine, off, 64);
  if (mine && (threadIdx.x & 63u) == 0) atomicAdd(n_one_way, (unsigned long long)mine);
}

// 5b. per rank r: is it a region's seed (size > 0), and is the region kept
__global__ __launch_bounds__(kRgBlock) void rg_flag_kernel(const uint32_t *__restrict__ rsz, uint32_t n_valid, uint32_t min_size, uint32_t max_size,
                                                           uint32_t *__restrict__ flag, uint32_t *__restrict__ n_regions) {
  const uint32_t r = blockIdx.x * kRgBlock + threadIdx.x;
  bool seed = false;
  if (r < n_valid) {
    const uint32_t sz = rsz[r];
    seed = sz > 0;
    flag[r] = (seed && sz >= min_size && sz <= max_size) ? 1u : 0u;
  }
  const unsigned long long m = __ballot(seed);
  if (m && (threadIdx.x & 63u) == 0) atomicAdd(n_regions, (uint32_t)__popcll(m));
}

// 5c. (rrank = exclusive scan of the flags) the kept regions' sizes in output order, K = their number
__global__ __launch_bounds__(kRgBlock) void rg_order_kernel(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ rrank,
                                                            const uint32_t *__restrict__ rsz, uint32_t n_valid, uint32_t *__restrict__ osize,
                                                            uint32_t *__restrict__ d_K) {
  const uint32_t r = blockIdx.x * kRgBlock + threadIdx.x;
  if (r >= n_valid) return;
  if (flag[r]) osize[rrank[r]] = rsz[r];
  if (r + 1 == n_valid) *d_K = rrank[r] + flag[r];
}

// 5d. per point (ORIGINAL order): the written region holding it or -1, and the key of the stable sort by region
__global__ __launch_bounds__(kRgBlock) void rg_label_kernel(const uint32_t *__restrict__ pos_by_o, const uint32_t *__restrict__ rank_of_pos,
                                                            const uint32_t *__restrict__ lab, const uint32_t *__restrict__ flag,
                                                            const uint32_t *__restrict__ rrank, uint32_t n, uint32_t n_valid, uint32_t kcap,
                                                            int32_t *__restrict__ label, uint32_t *__restrict__ lkey, uint32_t *__restrict__ lval) {
  const uint32_t o = blockIdx.x * kRgBlock + threadIdx.x;
  if (o >= n) return;
  const uint32_t p = pos_by_o[o];
  bool written = false;
  uint32_t rr = 0;
  if (p < n_valid) {
    const uint32_t l = lab[rank_of_pos[p]];
    if (flag[l]) { rr = rrank[l]; written = rr < kcap; }
  }
  label[o] = written ? (int32_t)rr : -1;
  lkey[o] = written ? rr : kcap;
  lval[o] = o;
}

struct Result {
  uint32_t K = 0;
  std::vector<uint32_t> off;
  size_t kw = 0;
};

int check_params(ope_ctx *ctx, const char *who, const ope_cloud *cloud, const ope_region_params *params, const float *normals, const float *curvature,
                 size_t *n_clusters, ope_region_params &p) {
  if (!ctx) return OPE_EINVAL;
  ctx->region_stats = ope_region_stats{};
  if (!cloud || !n_clusters) return set_err(ctx, OPE_EINVAL, std::string(who) + "bad argument");
  ope_region_default_params(&p);
  if (params) p = *params;
  if ((normals == nullptr) != (curvature == nullptr)) return set_err(ctx, OPE_EINVAL, std::string(who) + "pass normals and curvature, or neither");
  if (p.number_of_neighbours < 1 || p.number_of_neighbours > kKnnMaxK) return set_err(ctx, OPE_EINVAL, std::string(who) + "1 <= number_of_neighbours <= 32");
  if (!normals && (p.normals_k < 3 || p.normals_k > kKnnMaxK)) return set_err(ctx, OPE_EINVAL, std::string(who) + "3 <= normals_k <= 32");
  if (!std::isfinite(p.smoothness_threshold) || !std::isfinite((float)p.smoothness_threshold) || p.smoothness_threshold < 0.0)
    return set_err(ctx, OPE_EINVAL, std::string(who) + "smoothness_threshold must be finite and >= 0");
  if (!std::isfinite(p.curvature_threshold) || !std::isfinite((float)p.curvature_threshold))
    return set_err(ctx, OPE_EINVAL, std::string(who) + "curvature_threshold must be finite");
  if (p.min_size < 1) return set_err(ctx, OPE_EINVAL, std::string(who) + "min_size must be >= 1");
  if (p.max_size < p.min_size) return set_err(ctx, OPE_EINVAL, std::string(who) + "max_size < min_size");
  if (cloud->n > (size_t)0x7fffffff / (size_t)kKnnMaxK) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than (2^31 - 1) / 32 points");
  return OPE_OK;
}

// Steps 0-5.  On success the device buffers the _cloud form needs stay in tmp.
int region_core(ope_ctx *ctx, CallTmp &tmp, const char *who, ope_cloud *cloud, const ope_region_params &p, const float *normals, const float *curvature,
                size_t max_clusters, bool want_idx, int32_t *out_idx, int32_t *out_offsets, int32_t *out_label, Result &res,
                const int32_t **d_idx_out, const uint32_t **d_roff_out, const float4 **d_pts_out, const uint32_t **d_pos_out) {
  ope_region_stats &St = ctx->region_stats;
  const uint32_t n = (uint32_t)cloud->n, n_valid = (uint32_t)cloud->n_valid;
  const int k = p.number_of_neighbours;
  const float c = (float)std::cos((double)(float)p.smoothness_threshold);
  const float curv_thr = (float)p.curvature_threshold;
  const size_t kcap = std::min<size_t>(max_clusters, n);
  const int lbits = bits_for(kcap);
  const hipStream_t st = ctx->stream;
  // the normals: the caller's, or ope_normals' (which leaves them attached to the cloud)
  if (!normals) {
    const int rc = ope_normals(ctx, cloud, p.normals_k, nullptr, nullptr, nullptr);
    if (rc != OPE_OK) return rc;
  }
  hipError_t e = hipSuccess;
  const size_t nk = (size_t)std::max<uint32_t>(n_valid, 1) * (size_t)k;
  auto *pts_by_o = (float4 *)tmp.get(16ull * n, e);
  auto *pos_by_o = (uint32_t *)tmp.get(4ull * n, e);
  float4 *nrm_by_o = nullptr, *nrm_own = nullptr;
  if (normals) { nrm_by_o = (float4 *)tmp.get(16ull * n, e); nrm_own = (float4 *)tmp.get(16ull * n, e); }
  auto *keys = (unsigned long long *)tmp.get(8ull * n, e), *skey = (unsigned long long *)tmp.get(8ull * n, e);
  auto *vals = (uint32_t *)tmp.get(4ull * n, e), *sval = (uint32_t *)tmp.get(4ull * n, e);
  auto *rank_of_pos = (uint32_t *)tmp.get(4ull * n, e);
  auto *parent = (uint32_t *)tmp.get(4ull * n, e), *L = (uint32_t *)tmp.get(4ull * n, e);
  auto *adj = (uint32_t *)tmp.get(4ull * nk, e), *ow = (uint32_t *)tmp.get(4ull * nk, e);
  auto *self_leaf = (uint32_t *)tmp.get(4ull * n, e);
  auto *lab = (uint32_t *)tmp.get(4ull * n, e), *rsz = (uint32_t *)tmp.get(4ull * n, e);
  auto *flag = (uint32_t *)tmp.get(4ull * n, e), *rrank = (uint32_t *)tmp.get(4ull * n, e);
  auto *osize = (uint32_t *)tmp.get(4ull * (n + 1), e), *roff = (uint32_t *)tmp.get(4ull * (n + 1), e);
  auto *label = (int32_t *)tmp.get(4ull * n, e);
  auto *lkey = (uint32_t *)tmp.get(4ull * n, e), *lkey2 = (uint32_t *)tmp.get(4ull * n, e);
  auto *lval = (uint32_t *)tmp.get(4ull * n, e), *idx = (uint32_t *)tmp.get(4ull * n, e);
  // words: [0] refused, [1] regions, [2] K, [3] -, [4..5] one-way edges (64 bit), [8 .. 8 + kSweepBatch) the batch's change counters
  auto *words = (uint32_t *)tmp.get(64, e);
  size_t tb = 0, t1 = 0;
  if (e == hipSuccess) e = rocprim::radix_sort_pairs(nullptr, t1, keys, skey, vals, sval, n, 0, 64, st);
  tb = std::max(tb, t1);
  if (e == hipSuccess) e = rocprim::radix_sort_pairs(nullptr, t1, lkey, lkey2, lval, idx, n, 0, lbits, st);
  tb = std::max(tb, t1);
  if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, t1, osize, roff, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), st);
  tb = std::max(tb, t1);
  void *d_tmp = tmp.get(std::max<size_t>(tb, 16), e);
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  const CloudView cv = cloud->view();
  if (e == hipSuccess) e = hipMemsetAsync(words, 0, 64, st);
  if (e == hipSuccess) e = hipMemsetAsync(rsz, 0, 4ull * n, st);
  if (e == hipSuccess) e = hipMemsetAsync(osize, 0, 4ull * (n + 1), st);
  St.launches += 3;
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  // 0. positions; the caller's normals into the sorted order
  STAGE_LAUNCH(ctx, St.launches, rg_pos_kernel, 36.0 * n, dim3(grid_of(n, kRgBlock)), dim3(kRgBlock), 0, st, cv, pts_by_o, pos_by_o);
  const float4 *nrm = cloud->d_nrm;
  if (normals) {
    std::vector<float> packed(4ull * n);
    for (size_t i = 0; i < n; ++i) {
      packed[4 * i] = normals[3 * i]; packed[4 * i + 1] = normals[3 * i + 1]; packed[4 * i + 2] = normals[3 * i + 2];
      packed[4 * i + 3] = curvature[i];
    }
    e = h2d_copy(st, nrm_by_o, packed.data(), 16ull * n, &St.host_syncs);   // (a staged upload waits per chunk)
    if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
    STAGE_LAUNCH(ctx, St.launches, rg_gather_normals_kernel, 36.0 * n, dim3(grid_of(n, kRgBlock)), dim3(kRgBlock), 0, st, cv, nrm_by_o, nrm_own);
    nrm = nrm_own;
  }
  if (!nrm) return set_err(ctx, OPE_ESTATE, std::string(who) + "the cloud carries no normals");
  // 1. the refusal count, then the ranks
  STAGE_LAUNCH(ctx, St.launches, rg_key_kernel, 32.0 * n_valid, dim3(grid_of(n_valid, kRgBlock)), dim3(kRgBlock), 0, st, cv, nrm, curv_thr, keys, vals, words);
  uint32_t refused = 0;
  e = hipMemcpyAsync(&refused, words, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  ++St.host_syncs;
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  St.refused_curvature = (int64_t)refused;
  if (refused)
    return set_err(ctx, OPE_EINVAL, std::string(who) + std::to_string(refused) + " point(s) have a curvature above curvature_threshold: PCL's rule "
                   "for such points (labelled, not expanded unless a seed) is not built");
  uint64_t one_way = 0;
  int sweeps = 0;
  if (n_valid > 0) {
    STAGE_PRIM(ctx, St.launches, e, "rg_sort_ranks", rocprim::radix_sort_pairs(d_tmp, (t1 = tb), keys, skey, vals, sval, n_valid, 0, 64, st));
    STAGE_LAUNCH(ctx, St.launches, rg_rank_kernel, 16.0 * n_valid, dim3(grid_of(n_valid, kRgBlock)), dim3(kRgBlock), 0, st, sval, n_valid, rank_of_pos, parent,
                 L);
    if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
    // 2. the cloud's own tree, start leaves, the graph
    ope_index *ix = nullptr;
    ope_index_params ip;
    ope_index_default_params(&ip);
    ip.grid = 0;
    const int rc = index_build_tmp(ctx, cloud, &ip, &ix);
    if (rc != OPE_OK) return rc;
    struct FreeIx { ope_index *p; ~FreeIx() { ope_index_free(p); } } free_ix{ix};
    e = self_leaves(st, ix->view(), n, self_leaf);
    St.launches += 2;
    if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
    const unsigned gblocks = (unsigned)std::min<size_t>(((size_t)n_valid + kKnnBlock - 1) / kKnnBlock, 4096);
    if (k == 15)
      STAGE_LAUNCH_AS(ctx, St.launches, rg_graph_kernel<15>, "rg_graph_kernel", (double)n_valid * (16.0 + 36.0 * k), dim3(gblocks), dim3(kKnnBlock), 0, st, cv,
                      ix->view(), nrm, pos_by_o, self_leaf, k, c, adj);
    else
      STAGE_LAUNCH_AS(ctx, St.launches, rg_graph_kernel<0>, "rg_graph_kernel", (double)n_valid * (16.0 + 36.0 * k), dim3(gblocks), dim3(kKnnBlock),
                      kKnnLdsBytes, st, cv, ix->view(), nrm, pos_by_o, self_leaf, k, c, adj);
    // 3. mutual edges -> components
    STAGE_LAUNCH(ctx, St.launches, rg_mutual_kernel, (double)n_valid * 8.0 * k, dim3(grid_of(n_valid, kRgBlock)), dim3(kRgBlock), 0, st, adj, rank_of_pos,
                 n_valid, k, parent, ow, (unsigned long long *)(words + 4));
    STAGE_LAUNCH(ctx, St.launches, rg_flatten_kernel, 8.0 * n_valid, dim3(grid_of(n_valid, kRgBlock)), dim3(kRgBlock), 0, st, n_valid, parent);
    // 4. sweeps, four at a time, until one changes nothing
    for (bool done = false; !done;) {
      e = hipMemsetAsync(words + 8, 0, 4 * kSweepBatch, st);
      ++St.launches;
      if (e != hipSuccess) break;
      for (int s = 0; s < kSweepBatch; ++s)
        STAGE_LAUNCH(ctx, St.launches, rg_sweep_kernel, (double)n_valid * (12.0 + 4.0 * k), dim3(grid_of(n_valid, kRgBlock)), dim3(kRgBlock), 0, st, ow,
                     rank_of_pos, parent, n_valid, k, L, words + 8 + s);
      uint32_t hw[8 + kSweepBatch];
      e = hipMemcpyAsync(hw, words, sizeof hw, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      ++St.host_syncs;
      if (e != hipSuccess) break;
      one_way = (uint64_t)hw[4] | ((uint64_t)hw[5] << 32);
      for (int s = 0; s < kSweepBatch && !done; ++s) {
        ++sweeps;
        done = hw[8 + s] == 0;
      }
    }
    if (e != hipSuccess) { (void)hipStreamSynchronize(st); return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e)); }
    // 5. sizes, the filter, the order
    STAGE_LAUNCH(ctx, St.launches, rg_size_kernel, 16.0 * n_valid, dim3(grid_of(n_valid, kRgBlock)), dim3(kRgBlock), 0, st, parent, L, n_valid, lab, rsz);
    STAGE_LAUNCH(ctx, St.launches, rg_flag_kernel, 8.0 * n_valid, dim3(grid_of(n_valid, kRgBlock)), dim3(kRgBlock), 0, st, rsz, n_valid, (uint32_t)p.min_size,
                 (uint32_t)p.max_size, flag, words + 1);
    STAGE_PRIM(ctx, St.launches, e, "rg_scan_regions",
               rocprim::exclusive_scan(d_tmp, (t1 = tb), flag, rrank, 0u, (size_t)n_valid, rocprim::plus<uint32_t>(), st));
    STAGE_LAUNCH(ctx, St.launches, rg_order_kernel, 16.0 * n_valid, dim3(grid_of(n_valid, kRgBlock)), dim3(kRgBlock), 0, st, flag, rrank, rsz, n_valid, osize,
                 words + 2);
    // (the index goes back here; the stream's later work runs behind the walk that read it)
  }
  STAGE_PRIM(ctx, St.launches, e, "rg_scan_offsets", rocprim::exclusive_scan(d_tmp, (t1 = tb), osize, roff, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), st));
  STAGE_LAUNCH(ctx, St.launches, rg_label_kernel, 32.0 * n, dim3(grid_of(n, kRgBlock)), dim3(kRgBlock), 0, st, pos_by_o, rank_of_pos, lab, flag, rrank, n,
               n_valid, (uint32_t)kcap, label, lkey, lval);
  STAGE_PRIM(ctx, St.launches, e, "rg_sort_labels", rocprim::radix_sort_pairs(d_tmp, (t1 = tb), lkey, lkey2, lval, idx, n, 0, lbits, st));
  // the read-back: regions, K, offsets, indices, labels
  uint32_t hw[4] = {0, 0, 0, 0};
  std::vector<uint32_t> off(kcap + 1, 0);
  if (e == hipSuccess) e = hipMemcpyAsync(hw, words, 16, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(off.data(), roff, 4 * (kcap + 1), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && want_idx && n) e = hipMemcpyAsync(out_idx, idx, 4ull * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && out_label && n) e = hipMemcpyAsync(out_label, label, 4ull * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  ++St.host_syncs;
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  St.sweeps = sweeps;
  St.one_way_edges = (int64_t)one_way;
  St.regions_before_size_filter = (int64_t)hw[1];
  res.K = hw[2];
  res.kw = std::min<size_t>(res.K, kcap);
  off.resize(res.kw + 1);
  res.off = off;
  if (out_offsets)
    for (size_t q = 0; q <= res.kw; ++q) out_offsets[q] = (int32_t)off[q];
  *d_idx_out = (const int32_t *)idx;
  *d_roff_out = roff;
  *d_pts_out = pts_by_o;
  *d_pos_out = pos_by_o;
  return OPE_OK;
}

}  // namespace
}  // namespace ope

using namespace ope;

extern "C" {

void ope_region_default_params(ope_region_params *p) {
  if (!p) return;
  p->number_of_neighbours = 15;
  p->normals_k = 30;
  p->smoothness_threshold = 10.0 / 180.0 * M_PI;
  p->curvature_threshold = 1.0;
  p->min_size = 500;
  p->max_size = 1000000;
}

int ope_region_grow(ope_ctx *ctx, ope_cloud *cloud, const ope_region_params *params, const float *normals, const float *curvature, size_t max_clusters,
                    size_t *n_clusters, int32_t *out_idx, int32_t *out_offsets, int32_t *out_label) {
  static const char *who = "ope_region_grow: ";
  ope_region_params p;
  const int rc0 = check_params(ctx, who, cloud, params, normals, curvature, n_clusters, p);
  if (rc0 != OPE_OK) return rc0;
  if (max_clusters > 0 && (!out_idx || !out_offsets)) return set_err(ctx, OPE_EINVAL, std::string(who) + "out_idx and out_offsets are required");
  *n_clusters = 0;
  if (cloud->n == 0) { if (out_offsets) out_offsets[0] = 0; return OPE_OK; }
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  TraceRange r(ctx, "region_grow");
  CallTmp tmp{ctx->stream, {}};
  Result res;
  const int32_t *d_idx; const uint32_t *d_roff, *d_pos; const float4 *d_pts;
  const int rc = region_core(ctx, tmp, who, cloud, p, normals, curvature, max_clusters, max_clusters > 0, out_idx, out_offsets, out_label, res, &d_idx,
                             &d_roff, &d_pts, &d_pos);
  if (rc != OPE_OK) return rc;
  *n_clusters = res.K;
  return OPE_OK;
}

int ope_region_grow_cloud(ope_ctx *ctx, ope_cloud *cloud, const ope_region_params *params, const float *normals, const float *curvature,
                          size_t max_clusters, size_t *n_clusters, ope_cloud **out_clouds, int32_t *out_idx, int32_t *out_offsets) {
  static const char *who = "ope_region_grow_cloud: ";
  ope_region_params p;
  const int rc0 = check_params(ctx, who, cloud, params, normals, curvature, n_clusters, p);
  if (rc0 != OPE_OK) return rc0;
  if (max_clusters > 0 && !out_clouds) return set_err(ctx, OPE_EINVAL, std::string(who) + "out_clouds is required");
  *n_clusters = 0;
  if (cloud->n == 0) {
    for (size_t q = 0; q < max_clusters; ++q) out_clouds[q] = nullptr;
    if (out_offsets) out_offsets[0] = 0;
    return OPE_OK;
  }
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  TraceRange r(ctx, "region_grow");
  CallTmp tmp{ctx->stream, {}};
  Result res;
  const int32_t *d_idx; const uint32_t *d_roff, *d_pos; const float4 *d_pts;
  int rc = region_core(ctx, tmp, who, cloud, p, normals, curvature, max_clusters, out_idx != nullptr, out_idx, out_offsets, nullptr, res, &d_idx, &d_roff,
                       &d_pts, &d_pos);
  if (rc != OPE_OK) return rc;
  for (size_t q = 0; q < max_clusters; ++q) out_clouds[q] = nullptr;
  if (res.kw > 0) {
    rc = clusters_build_clouds(ctx, tmp, who, cloud, res.kw, res.off, d_idx, d_roff, d_pts, d_pos, out_clouds, &ctx->region_stats.launches,
                               &ctx->region_stats.host_syncs);
    if (rc != OPE_OK) return rc;
  }
  *n_clusters = res.K;
  return OPE_OK;
}

int ope_region_last_stats(const ope_ctx *ctx, ope_region_stats *out) {
  if (!ctx || !out) return OPE_EINVAL;
  *out = ctx->region_stats;
  return OPE_OK;
}

}  // extern "C"
