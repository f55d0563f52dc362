// region_grow_rgb.hip — colour-based region growing on the device (ope_region_grow_rgb, gfx950, wave64): what pcl::RegionGrowingRGB
// returns as SegmentationRegionGrow::getSegmentRegGrowRgb runs it (segmentationregiongrow.cpp:85-151; normal, curvature and residual
// tests off).  DESIGN.md §4.19 has the restatement and the proof of the parallel form of the first merge pass.
//
//   1. rank: the index of a point among the finite points by ORIGINAL index (a scan; seeds go by original index);
//   2. search (the hot kernel): one lane per finite point walks the cloud's own tree from the point's own leaf for its K nearest
//      (K up to 128, PCL's 100) and writes their sorted positions and squared distances in rows, and the row's largest distance.
//      The list lives in LDS, UNSORTED, with its maximum tracked: only the K-th distance prunes, and the order is never used.
//      Workgroups of 64 lanes: 64 x K x 8 B of list (50 KiB at K = 100) + the walk's stack, checked against the device's limit;
//   3. point edges u -> v: v in N(u), v != u, !(cd(u, v) > P2).  The colour test is symmetric, so the edge is mutual iff u is in
//      N(v): d2 below v's row maximum (a row scan only on equality).  Mutual edges -> union-find, the others are "one-way";
//   4. the sweeps of region_grow.hip (four per batch, one read-back per batch) -> segment(v) = smallest rank that reaches v;
//   5. segments: dense numbers by a scan over the seeds, sizes and the three integer colour sums by wave-aggregated atomics;
//   6. segment pairs: every row entry whose ends lie in different segments gives (seg u, seg v) -> d2; radix sort by the pair,
//      minimum per pair, a second (stable) sort by (seg u, d2), and the first K per segment kept in S x K tables;
//   7. one download of the kept tables (S x K x 8 B), the sizes and the sums; the merges on the host: merge A by the parent
//      formula, merge B a sequential replay over the regions, PCL's two-pointer order, the size filter;
//   8. one upload of the cluster of every segment and the offsets; labels and a stable sort of the ORIGINAL indices by cluster.
// Kernel launches booked: 27 + 5 per batch of four sweeps (+ 5 for the _cloud form); host synchronisations: 4 + 1 per batch (+ 1
// for the _cloud form).  The build of the cloud's tree is not booked.  Neither count depends on the number of points, segments
// or regions.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "bvh_traverse.hpp"
#include "coarse_stages.hpp"
#include "region_common.hpp"
#include "stage_host.hpp"

namespace ope {

namespace {

constexpr int kRgbMaxK = 128;
constexpr int kRgbLanes = 64;   // one wave per workgroup: the lists of 64 lanes are what fits
constexpr unsigned long long kNoPair = ~0ull;

// k-nearest list of one lane in LDS with a per-lane stride, UNSORTED: a candidate replaces the list's maximum and the new maximum
// is found by one pass over the k entries.  (KnnVisitor's sorted insertion shifts up to k entries per candidate.)
struct KnnBagVisitor {
  float *d;
  uint32_t *pos;
  int k, count, worst_j;
  float worst;
  __device__ __forceinline__ bool prune(float bound) const { return !(bound < worst); }
  __device__ __forceinline__ void point(float dist, const v4f &, uint32_t i, uint32_t) {
    if (!(dist < worst)) return;
    if (count < k) {
      d[count * kRgbLanes] = dist;
      pos[count * kRgbLanes] = i;
      if (++count < k) return;
    } else {
      d[worst_j * kRgbLanes] = dist;
      pos[worst_j * kRgbLanes] = i;
    }
    float m = d[0];
    int mj = 0;
    for (int j = 1; j < k; ++j) {
      const float x = d[j * kRgbLanes];
      if (x > m) { m = x; mj = j; }
    }
    worst = m;
    worst_j = mj;
  }
  __device__ __forceinline__ void on_node() {}
};

// 1. is the point of ORIGINAL index o finite
__global__ __launch_bounds__(kRgBlock) void rgb_finite_kernel(const uint32_t *__restrict__ pos_by_o, uint32_t n, uint32_t n_valid, uint32_t *__restrict__ fin) {
  const uint32_t o = blockIdx.x * kRgBlock + threadIdx.x;
  if (o < n) fin[o] = pos_by_o[o] < n_valid ? 1u : 0u;
}
// (frank = exclusive scan of fin) rank of every sorted position; a point's own parent and label
__global__ __launch_bounds__(kRgBlock) void rgb_rank_kernel(CloudView c, const uint32_t *__restrict__ frank, uint32_t *__restrict__ rank_of_pos,
                                                            uint32_t *__restrict__ parent, uint32_t *__restrict__ L) {
  const uint32_t p = blockIdx.x * kRgBlock + threadIdx.x;
  if (p >= c.n_valid) return;
  const uint32_t r = frank[(uint32_t)__float_as_int(c.xyzw[p].w)];
  rank_of_pos[p] = r;
  parent[r] = r;
  L[r] = r;
}

// 2. the search.  Dynamic LDS: k x 64 distances, k x 64 positions, (kMaxDepth + 1) x 64 parked bounds.
__global__ __launch_bounds__(kRgbLanes) void rgb_search_kernel(CloudView q, BvhView tgt, const uint32_t *__restrict__ pos_by_o,
                                                               const uint32_t *__restrict__ self_leaf, int k, uint32_t *__restrict__ nbr,
                                                               float *__restrict__ nd2, float *__restrict__ rowmax) {
  extern __shared__ __align__(16) unsigned char s_dyn[];
  float *ld = reinterpret_cast<float *>(s_dyn) + threadIdx.x;
  uint32_t *lp = reinterpret_cast<uint32_t *>(s_dyn) + (size_t)k * kRgbLanes + threadIdx.x;
  float *stk = reinterpret_cast<float *>(s_dyn) + 2 * (size_t)k * kRgbLanes + threadIdx.x;
  for (uint32_t base = blockIdx.x * kRgbLanes; base < q.n_valid; base += gridDim.x * kRgbLanes) {
    const uint32_t i = base + threadIdx.x;
    const bool active = i < q.n_valid;
    const float4 s = q.xyzw[active ? i : 0];
    const uint32_t h = active ? self_leaf[(uint32_t)__float_as_int(s.w)] : 0u;
    KnnBagVisitor v{ld, lp, k, 0, 0, active ? INFINITY : -INFINITY};
    if (active) bvh_traverse(tgt, s.x, s.y, s.z, v, stk, kRgbLanes, h);
    if (active) {
      uint32_t *row = nbr + (size_t)i * (size_t)k;
      float *rd = nd2 + (size_t)i * (size_t)k;
      for (int j = 0; j < k; ++j) {
        const bool has = j < v.count;
        row[j] = has ? pos_by_o[(uint32_t)__float_as_int(tgt.pts[lp[j * kRgbLanes]].w)] : kNone;
        rd[j] = has ? ld[j * kRgbLanes] : INFINITY;
      }
      rowmax[i] = v.count == k ? v.worst : INFINITY;   // (a short row holds every finite point)
    }
  }
}

// PCL's calculateColorimetricalDifference on two colour words
__device__ __host__ __forceinline__ uint32_t color_dist(uint32_t a, uint32_t b) {
  const int dr = (int)((a >> 16) & 255u) - (int)((b >> 16) & 255u), dg = (int)((a >> 8) & 255u) - (int)((b >> 8) & 255u),
            db = (int)(a & 255u) - (int)(b & 255u);
  return (uint32_t)(dr * dr + dg * dg + db * db);
}

// 3. per point u (a sorted position) and row entry v: an edge iff v != u and !(cd > P2); mutual -> one union of the two ranks,
// made from the smaller end; otherwise kept in ow (one-way, v as its rank) and counted
__global__ __launch_bounds__(kRgBlock) void rgb_edges_kernel(const uint32_t *__restrict__ nbr, const float *__restrict__ nd2, const float *__restrict__ rowmax,
                                                             const uint32_t *__restrict__ rgb, const uint32_t *__restrict__ rank_of_pos, uint32_t n_valid,
                                                             int k, float p2, uint32_t *__restrict__ parent, uint32_t *__restrict__ ow,
                                                             unsigned long long *__restrict__ n_one_way) {
  const uint32_t u = blockIdx.x * kRgBlock + threadIdx.x;
  uint32_t mine = 0;
  if (u < n_valid) {
    const uint32_t cu = rgb[u];
    for (int j = 0; j < k; ++j) {
      const uint32_t v = nbr[(size_t)u * k + j];
      uint32_t keep = kNone;
      if (v != kNone && v != u && !((float)color_dist(cu, rgb[v]) > p2)) {
        const float d = nd2[(size_t)u * k + j], m = rowmax[v];
        bool mutual = d < m;
        if (!mutual && d == m)
          for (int t = 0; t < k; ++t) mutual |= nbr[(size_t)v * k + t] == u;
        if (mutual) { if (u < v) uf_union(parent, rank_of_pos[u], rank_of_pos[v]); }
        else { keep = rank_of_pos[v]; ++mine; }
      }
      ow[(size_t)u * k + j] = keep;
    }
  }
  for (int off = 32; off >= 1; off >>= 1) mine += (uint32_t)__shfl_xor((int)mine, off, 64);
  if (mine && (threadIdx.x & 63u) == 0) atomicAdd(n_one_way, (unsigned long long)mine);
}

// 5a. per rank r: is it a segment's seed
__global__ __launch_bounds__(kRgBlock) void rgb_seed_kernel(const uint32_t *__restrict__ rsz, uint32_t n_valid, uint32_t *__restrict__ flag) {
  const uint32_t r = blockIdx.x * kRgBlock + threadIdx.x;
  if (r < n_valid) flag[r] = rsz[r] > 0 ? 1u : 0u;
}
// 5b. (segno = exclusive scan of the seed flags) per sorted position its dense segment; per segment the size and the channel sums
// (stat[4 s ..] = count, r, g, b), summed per wave and segment before the atomics; words[0] = S
__global__ __launch_bounds__(kRgBlock) void rgb_stats_kernel(const uint32_t *__restrict__ rank_of_pos, const uint32_t *__restrict__ lab,
                                                             const uint32_t *__restrict__ segno, const uint32_t *__restrict__ flag,
                                                             const uint32_t *__restrict__ rgb, uint32_t n_valid, uint32_t *__restrict__ seg_of_pos,
                                                             uint32_t *__restrict__ stat, uint32_t *__restrict__ words) {
  const uint32_t p = blockIdx.x * kRgBlock + threadIdx.x;
  const bool on = p < n_valid;
  uint32_t s = kNone, c = 0;
  if (on) {
    s = segno[lab[rank_of_pos[p]]];
    seg_of_pos[p] = s;
    c = rgb[p];
    if (p + 1 == n_valid) words[0] = segno[n_valid - 1] + flag[n_valid - 1];   // (by rank: the last rank's number, + 1 if it is a seed)
  }
  unsigned long long left = __ballot(on);
  while (left) {
    const int leader = __ffsll((long long)left) - 1;
    const uint32_t r = (uint32_t)__shfl((int)s, leader, 64);
    const bool in = on && s == r;
    const unsigned long long grp = __ballot(in);
    uint32_t sr = in ? (c >> 16) & 255u : 0u, sg = in ? (c >> 8) & 255u : 0u, sb = in ? c & 255u : 0u;
    for (int off = 32; off >= 1; off >>= 1) {
      sr += (uint32_t)__shfl_xor((int)sr, off, 64);
      sg += (uint32_t)__shfl_xor((int)sg, off, 64);
      sb += (uint32_t)__shfl_xor((int)sb, off, 64);
    }
    if ((int)(threadIdx.x & 63u) == leader) {
      atomicAdd(stat + 4 * (size_t)r, (uint32_t)__popcll(grp));
      atomicAdd(stat + 4 * (size_t)r + 1, sr);
      atomicAdd(stat + 4 * (size_t)r + 2, sg);
      atomicAdd(stat + 4 * (size_t)r + 3, sb);
    }
    left &= ~grp;
  }
}

// 6a. per row entry: (seg u << 32 | seg v) -> the bits of d2 (d2 >= 0: the unsigned order is the float order); kNoPair elsewhere
__global__ __launch_bounds__(kRgBlock) void rgb_pair_keys_kernel(const uint32_t *__restrict__ nbr, const float *__restrict__ nd2,
                                                                 const uint32_t *__restrict__ seg_of_pos, size_t total, int k,
                                                                 unsigned long long *__restrict__ keys, uint32_t *__restrict__ vals) {
  const size_t e = (size_t)blockIdx.x * kRgBlock + threadIdx.x;
  if (e >= total) return;
  const uint32_t v = nbr[e];
  unsigned long long key = kNoPair;
  if (v != kNone) {
    const uint32_t su = seg_of_pos[e / (size_t)k], sv = seg_of_pos[v];
    if (su != sv) key = ((unsigned long long)su << 32) | sv;
  }
  keys[e] = key;
  vals[e] = (uint32_t)__float_as_int(nd2[e]);
}
// 6b. words[1] = P, the number of directed pairs: the runs of the reduction without the run of kNoPair
__global__ void rgb_pair_count_kernel(const unsigned long long *__restrict__ ukeys, const uint32_t *__restrict__ n_runs, uint32_t *__restrict__ words) {
  const uint32_t u = *n_runs;
  words[1] = u - ((u > 0 && ukeys[u - 1] == kNoPair) ? 1u : 0u);
}
// 6c. the second sort's key (seg u << 32 | d2 bits) and value (seg v); the pairs come sorted by (seg u, seg v) and the sort is
// stable, so equal distances stay in ascending seg v: the order of std::priority_queue over (dist, t)
__global__ __launch_bounds__(kRgBlock) void rgb_pair_rekey_kernel(const unsigned long long *__restrict__ ukeys, const uint32_t *__restrict__ umin, uint32_t np,
                                                                  unsigned long long *__restrict__ keys, uint32_t *__restrict__ vals) {
  const uint32_t i = blockIdx.x * kRgBlock + threadIdx.x;
  if (i >= np) return;
  const unsigned long long key = ukeys[i];
  keys[i] = (key & 0xffffffff00000000ull) | umin[i];
  vals[i] = (uint32_t)key;
}
// 6d. first sorted pair of every segment that has one
__global__ __launch_bounds__(kRgBlock) void rgb_pair_start_kernel(const unsigned long long *__restrict__ keys, uint32_t np, uint32_t *__restrict__ start) {
  const uint32_t i = blockIdx.x * kRgBlock + threadIdx.x;
  if (i >= np) return;
  const uint32_t s = (uint32_t)(keys[i] >> 32);
  if (i == 0 || (uint32_t)(keys[i - 1] >> 32) != s) start[s] = i;
}
// 6e. the first k pairs of every segment into its row of the kept tables; kept_n[s] = their number (zeroed before)
__global__ __launch_bounds__(kRgBlock) void rgb_pair_keep_kernel(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t np,
                                                                 const uint32_t *__restrict__ start, int k, uint32_t *__restrict__ kept_d,
                                                                 uint32_t *__restrict__ kept_t, uint32_t *__restrict__ kept_n) {
  const uint32_t i = blockIdx.x * kRgBlock + threadIdx.x;
  if (i >= np) return;
  const uint32_t s = (uint32_t)(keys[i] >> 32), r = i - start[s];
  if (r >= (uint32_t)k) return;
  kept_d[(size_t)s * k + r] = (uint32_t)keys[i];
  kept_t[(size_t)s * k + r] = vals[i];
  if (r + 1 == (uint32_t)k || i + 1 == np || (uint32_t)(keys[i + 1] >> 32) != s) kept_n[s] = r + 1;
}

// 8. per point (ORIGINAL order): the written cluster holding it or -1, and the key of the stable sort by cluster
__global__ __launch_bounds__(kRgBlock) void rgb_label_kernel(const uint32_t *__restrict__ pos_by_o, const uint32_t *__restrict__ seg_of_pos,
                                                             const int32_t *__restrict__ cluster_of_seg, uint32_t n, uint32_t n_valid, uint32_t kcap,
                                                             int32_t *__restrict__ label, uint32_t *__restrict__ lkey, uint32_t *__restrict__ lval) {
  const uint32_t o = blockIdx.x * kRgBlock + threadIdx.x;
  if (o >= n) return;
  const uint32_t p = pos_by_o[o];
  int32_t c = -1;
  if (p < n_valid) c = cluster_of_seg[seg_of_pos[p]];
  const bool written = c >= 0 && (uint32_t)c < kcap;
  label[o] = written ? c : -1;
  lkey[o] = written ? (uint32_t)c : kcap;
  lval[o] = o;
}

struct Result {
  uint32_t K = 0;
  std::vector<uint32_t> off;
  size_t kw = 0;
};

// What the host works on: per segment its size, channel sums and kept neighbours (kept_n[s] entries of row s, ascending (dist, t))
struct Segments {
  size_t S = 0;
  int k = 0;
  std::vector<uint32_t> stat, kept_d, kept_t, kept_n;
};

struct DistSeg {
  float d;
  uint32_t s;
  bool operator<(const DistSeg &o) const { return d < o.d || (d == o.d && s < o.s); }
};

// Steps 5 (means) and 7 to 10 of the restatement: the cluster of every segment (-1: dropped) and the clusters' sizes in output order
void merge_segments(const Segments &g, float d2_thr, float r2_thr, uint32_t min_size, uint32_t max_size, std::vector<int32_t> &cluster_of_seg,
                    std::vector<uint32_t> &cluster_size, ope_region_rgb_stats &stats) {
  const size_t S = g.S;
  const int k = g.k;
  std::vector<uint32_t> mean(S);
  for (size_t s = 0; s < S; ++s) {
    const float cnt = (float)g.stat[4 * s];
    uint32_t m = 0;
    for (int c = 0; c < 3; ++c) m = (m << 8) | ((uint32_t)((float)g.stat[4 * s + 1 + c] / cnt) & 255u);
    mean[s] = m;
  }
  auto dist_of = [&](size_t s, uint32_t e) { float d; std::memcpy(&d, &g.kept_d[s * k + e], 4); return d; };
  // merge A: parent(x) = the smallest i < x that keeps x within the distance threshold and has a similar mean; region = the root
  std::vector<int64_t> par(S, -1);
  for (size_t i = 0; i < S; ++i)
    for (uint32_t e = 0; e < g.kept_n[i]; ++e) {
      const uint32_t x = g.kept_t[i * k + e];
      if (x > i && par[x] < 0 && !(dist_of(i, e) > d2_thr) && (float)color_dist(mean[i], mean[x]) < r2_thr) par[x] = (int64_t)i;
    }
  std::vector<uint32_t> reg(S);
  std::vector<std::vector<uint32_t>> members;
  std::vector<uint64_t> count;
  for (size_t x = 0; x < S; ++x) {
    if (par[x] < 0) { reg[x] = (uint32_t)members.size(); members.emplace_back(); count.push_back(0); }
    else reg[x] = reg[(size_t)par[x]];
    members[reg[x]].push_back((uint32_t)x);
    count[reg[x]] += g.stat[4 * x];
  }
  const size_t H = members.size();
  stats.homogeneous_regions = (int64_t)H;
  // region neighbours
  std::vector<std::vector<DistSeg>> lists(H);
  for (size_t r = 0; r < H; ++r) {
    for (uint32_t s : members[r])
      for (uint32_t e = 0; e < g.kept_n[s]; ++e) {
        const uint32_t x = g.kept_t[(size_t)s * k + e];
        if (reg[x] != r) lists[r].push_back(DistSeg{dist_of(s, e), x});
      }
    std::sort(lists[r].begin(), lists[r].end());
  }
  // merge B: sequential, in the state the earlier merges of this loop left
  int64_t absorbed = 0;
  for (size_t r = 0; r < H; ++r) {
    if (count[r] >= min_size) continue;
    if (lists[r].empty() || lists[r][0].d == FLT_MAX) continue;
    const uint32_t q = reg[lists[r][0].s];
    for (uint32_t s : members[r]) { reg[s] = q; members[q].push_back(s); }
    members[r].clear();
    count[q] += count[r];
    count[r] = 0;
    for (DistSeg &e : lists[q])
      if (reg[e.s] == q) e = DistSeg{FLT_MAX, 0};
    for (const DistSeg &e : lists[r])
      if (reg[e.s] != q) lists[q].push_back(e);
    lists[r].clear();
    std::sort(lists[q].begin(), lists[q].end());
    ++absorbed;
  }
  stats.regions_absorbed = absorbed;
  // PCL's two-pointer pass over the regions, then the size filter
  std::vector<uint32_t> order(H);
  for (size_t r = 0; r < H; ++r) order[r] = (uint32_t)r;
  if (H > 0)
    for (size_t i = 0, j = H - 1; i < j;) {
      while (i < j && count[order[i]] > 0) ++i;
      while (i < j && count[order[j]] == 0) --j;
      if (i != j) std::swap(order[i], order[j]);
    }
  std::vector<int32_t> cluster_of_reg(H, -1);
  cluster_size.clear();
  int64_t nonempty = 0;
  for (size_t q = 0; q < H; ++q) {
    const uint64_t c = count[order[q]];
    nonempty += c > 0;
    if (c < min_size || c > max_size) continue;
    cluster_of_reg[order[q]] = (int32_t)cluster_size.size();
    cluster_size.push_back((uint32_t)c);
  }
  stats.regions_before_size_filter = nonempty;
  cluster_of_seg.resize(S);
  for (size_t s = 0; s < S; ++s) cluster_of_seg[s] = cluster_of_reg[reg[s]];
}

int check_params(ope_ctx *ctx, const char *who, const ope_cloud *cloud, const ope_region_rgb_params *params, size_t *n_clusters, ope_region_rgb_params &p) {
  if (!ctx) return OPE_EINVAL;
  ctx->region_rgb_stats = ope_region_rgb_stats{};
  if (!cloud || !n_clusters) return set_err(ctx, OPE_EINVAL, std::string(who) + "bad argument");
  ope_region_rgb_default_params(&p);
  if (params) p = *params;
  if (!cloud->d_rgb) return set_err(ctx, OPE_EINVAL, std::string(who) + "the cloud has no colours");
  if (p.region_neighbour_number < 1 || p.region_neighbour_number > kRgbMaxK)
    return set_err(ctx, OPE_EINVAL, std::string(who) + "1 <= region_neighbour_number <= 128");
  for (double t : {p.distance_threshold, p.point_color_threshold, p.region_color_threshold})
    if (!std::isfinite(t) || !std::isfinite((float)t) || t < 0.0) return set_err(ctx, OPE_EINVAL, std::string(who) + "thresholds must be finite and >= 0");
  if (p.min_size < 1) return set_err(ctx, OPE_EINVAL, std::string(who) + "min_size must be >= 1");
  if (p.max_size < p.min_size) return set_err(ctx, OPE_EINVAL, std::string(who) + "max_size < min_size");
  if (cloud->n > (size_t)0x7fffffff / (size_t)kRgbMaxK) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than (2^31 - 1) / 128 points");
  return OPE_OK;
}

#define RGB_CHECK()                                                                              \
  do {                                                                                           \
    if (e == hipSuccess) e = hipGetLastError();                                                  \
    if (e != hipSuccess) { (void)hipStreamSynchronize(st); return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e)); } \
  } while (0)

// Steps 1-8.  On success the device buffers the _cloud form needs stay in tmp.
int region_rgb_core(ope_ctx *ctx, CallTmp &tmp, const char *who, const ope_cloud *cloud, const ope_region_rgb_params &p, size_t max_clusters, bool want_idx,
                    int32_t *out_idx, int32_t *out_offsets, int32_t *out_label, Result &res, const int32_t **d_idx_out, const uint32_t **d_roff_out,
                    const float4 **d_pts_out, const uint32_t **d_pos_out) {
  ope_region_rgb_stats &stats = ctx->region_rgb_stats;
  const uint32_t n = (uint32_t)cloud->n, n_valid = (uint32_t)cloud->n_valid;
  const int k = p.region_neighbour_number;
  const float fd = (float)p.distance_threshold, fp = (float)p.point_color_threshold, fr = (float)p.region_color_threshold;
  const float d2_thr = fd * fd, p2_thr = fp * fp, r2_thr = fr * fr;
  const size_t kcap = std::min<size_t>(max_clusters, n);
  const int lbits = bits_for(kcap);
  const int sbits = bits_for(std::max<uint32_t>(n_valid, 1));
  const hipStream_t st = ctx->stream;
  // the search's LDS against what a workgroup may have on this device
  const size_t lds = sizeof(float) * kRgbLanes * (2 * (size_t)k + kMaxDepth + 1);
  int lds_max = 0;
  hipError_t e = hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device);
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  if (lds > (size_t)lds_max)
    return set_err(ctx, OPE_ESTATE, std::string(who) + "the neighbour lists need " + std::to_string(lds) + " bytes of LDS per workgroup, the device allows " +
                   std::to_string(lds_max));
  if (lds > 65536) {
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(rgb_search_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  }
  const size_t nv1 = std::max<uint32_t>(n_valid, 1);
  const size_t nk = nv1 * (size_t)k;
  auto *pts_by_o = (float4 *)tmp.get(16ull * n, e);
  auto *pos_by_o = (uint32_t *)tmp.get(4ull * n, e);
  auto *fin = (uint32_t *)tmp.get(4ull * n, e), *frank = (uint32_t *)tmp.get(4ull * n, e);
  auto *rank_of_pos = (uint32_t *)tmp.get(4ull * n, e);
  auto *parent = (uint32_t *)tmp.get(4ull * n, e), *L = (uint32_t *)tmp.get(4ull * n, e);
  auto *nbr = (uint32_t *)tmp.get(4ull * nk, e), *ow = (uint32_t *)tmp.get(4ull * nk, e);
  auto *nd2 = (float *)tmp.get(4ull * nk, e), *rowmax = (float *)tmp.get(4ull * n, e);
  auto *self_leaf = (uint32_t *)tmp.get(4ull * n, e);
  auto *lab = (uint32_t *)tmp.get(4ull * n, e), *rsz = (uint32_t *)tmp.get(4ull * n, e);
  auto *flag = (uint32_t *)tmp.get(4ull * n, e), *segno = (uint32_t *)tmp.get(4ull * n, e);
  auto *seg_of_pos = (uint32_t *)tmp.get(4ull * n, e), *stat = (uint32_t *)tmp.get(16ull * nv1, e);
  auto *pkey = (unsigned long long *)tmp.get(8ull * nk, e), *pkey2 = (unsigned long long *)tmp.get(8ull * nk, e);
  auto *pval = (uint32_t *)tmp.get(4ull * nk, e), *pval2 = (uint32_t *)tmp.get(4ull * nk, e);
  auto *pstart = (uint32_t *)tmp.get(4ull * nv1, e), *kept_n = (uint32_t *)tmp.get(4ull * nv1, e);
  auto *label = (int32_t *)tmp.get(4ull * n, e);
  auto *lkey = (uint32_t *)tmp.get(4ull * n, e), *lkey2 = (uint32_t *)tmp.get(4ull * n, e);
  auto *lval = (uint32_t *)tmp.get(4ull * n, e), *idx = (uint32_t *)tmp.get(4ull * n, e);
  // one upload: the cluster of every segment, then the kcap + 1 offsets
  auto *d_up = (uint32_t *)tmp.get(4ull * (nv1 + kcap + 1), e);
  // words: [0] S, [1] P, [2] the reduction's runs, [4..5] one-way edges (64 bit), [8 .. 8 + kSweepBatch) the batch's change counters
  auto *words = (uint32_t *)tmp.get(64, e);
  size_t tb = 0, t1 = 0;
  if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, t1, fin, frank, 0u, (size_t)n, rocprim::plus<uint32_t>(), st);
  tb = std::max(tb, t1);
  if (e == hipSuccess) e = rocprim::radix_sort_pairs(nullptr, t1, pkey, pkey2, pval, pval2, nk, 0, 64, st);
  tb = std::max(tb, t1);
  if (e == hipSuccess)
    e = rocprim::reduce_by_key(nullptr, t1, pkey2, pval2, nk, pkey, pval, words + 2, rocprim::minimum<uint32_t>(), rocprim::equal_to<unsigned long long>(), st);
  tb = std::max(tb, t1);
  if (e == hipSuccess) e = rocprim::radix_sort_pairs(nullptr, t1, lkey, lkey2, lval, idx, n, 0, lbits, st);
  tb = std::max(tb, t1);
  void *d_tmp = tmp.get(std::max<size_t>(tb, 16), e);
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  const CloudView cv = cloud->view();
  if (e == hipSuccess) e = hipMemsetAsync(words, 0, 64, st);
  if (e == hipSuccess) e = hipMemsetAsync(rsz, 0, 4ull * n, st);
  if (e == hipSuccess) e = hipMemsetAsync(stat, 0, 16ull * nv1, st);
  if (e == hipSuccess) e = hipMemsetAsync(kept_n, 0, 4ull * nv1, st);
  stats.launches += 4;
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
  STAGE_LAUNCH(ctx, stats.launches, rg_pos_kernel, 36.0 * n, dim3(grid_of(n, kRgBlock)), dim3(kRgBlock), 0, st, cv, pts_by_o, pos_by_o);
  std::vector<int32_t> cluster_of_seg;
  std::vector<uint32_t> cluster_size;
  uint64_t one_way = 0;
  int sweeps = 0;
  uint32_t S = 0;
  if (n_valid > 0) {
    // 1. ranks
    STAGE_LAUNCH(ctx, stats.launches, rgb_finite_kernel, 8.0 * n, dim3(grid_of(n, kRgBlock)), dim3(kRgBlock), 0, st, pos_by_o, n, n_valid, fin);
    STAGE_PRIM(ctx, stats.launches, e, "rgb_scan_ranks", rocprim::exclusive_scan(d_tmp, (t1 = tb), fin, frank, 0u, (size_t)n, rocprim::plus<uint32_t>(), st));
    STAGE_LAUNCH(ctx, stats.launches, rgb_rank_kernel, 32.0 * n_valid, dim3(grid_of(n_valid, kRgBlock)), dim3(kRgBlock), 0, st, cv, frank, rank_of_pos, parent,
                 L);
    RGB_CHECK();
    // 2. the cloud's own tree, start leaves, the search
    ope_index *ix = nullptr;
    ope_index_params ip;
    ope_index_default_params(&ip);
    ip.grid = 0;
    const int rc = index_build_tmp(ctx, cloud, &ip, &ix);
    if (rc != OPE_OK) return rc;
    struct FreeIx { ope_index *p; ~FreeIx() { ope_index_free(p); } } free_ix{ix};
    e = self_leaves(st, ix->view(), n, self_leaf);
    stats.launches += 2;
    RGB_CHECK();
    const unsigned sblocks = (unsigned)std::min<size_t>(((size_t)n_valid + kRgbLanes - 1) / kRgbLanes, 16384);
    STAGE_LAUNCH(ctx, stats.launches, rgb_search_kernel, (double)n_valid * (20.0 + 24.0 * k), dim3(sblocks), dim3(kRgbLanes), lds, st, cv, ix->view(), pos_by_o,
                 self_leaf, k, nbr, nd2, rowmax);
    // 3. edges -> components
    STAGE_LAUNCH(ctx, stats.launches, rgb_edges_kernel, (double)n_valid * 16.0 * k, dim3(grid_of(n_valid, kRgBlock)), dim3(kRgBlock), 0, st, nbr, nd2, rowmax,
                 cloud->d_rgb, rank_of_pos, n_valid, k, p2_thr, parent, ow, (unsigned long long *)(words + 4));
    STAGE_LAUNCH(ctx, stats.launches, rg_flatten_kernel, 8.0 * n_valid, dim3(grid_of(n_valid, kRgBlock)), dim3(kRgBlock), 0, st, n_valid, parent);
    RGB_CHECK();
    // 4. sweeps, four at a time, until one changes nothing
    for (bool done = false; !done;) {
      e = hipMemsetAsync(words + 8, 0, 4 * kSweepBatch, st);
      ++stats.launches;
      if (e != hipSuccess) break;
      for (int s = 0; s < kSweepBatch; ++s)
        STAGE_LAUNCH(ctx, stats.launches, rg_sweep_kernel, (double)n_valid * (12.0 + 4.0 * k), dim3(grid_of(n_valid, kRgBlock)), dim3(kRgBlock), 0, st, ow,
                     rank_of_pos, parent, n_valid, k, L, words + 8 + s);
      uint32_t hw[8 + kSweepBatch];
      e = hipMemcpyAsync(hw, words, sizeof hw, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      ++stats.host_syncs;
      if (e != hipSuccess) break;
      one_way = (uint64_t)hw[4] | ((uint64_t)hw[5] << 32);
      for (int s = 0; s < kSweepBatch && !done; ++s) {
        ++sweeps;
        done = hw[8 + s] == 0;
      }
    }
    RGB_CHECK();
    // 5. segments: label per rank, sizes by seed rank, dense numbers, colour sums
    STAGE_LAUNCH(ctx, stats.launches, rg_size_kernel, 16.0 * n_valid, dim3(grid_of(n_valid, kRgBlock)), dim3(kRgBlock), 0, st, parent, L, n_valid, lab, rsz);
    STAGE_LAUNCH(ctx, stats.launches, rgb_seed_kernel, 8.0 * n_valid, dim3(grid_of(n_valid, kRgBlock)), dim3(kRgBlock), 0, st, rsz, n_valid, flag);
    STAGE_PRIM(ctx, stats.launches, e, "rgb_scan_segments",
               rocprim::exclusive_scan(d_tmp, (t1 = tb), flag, segno, 0u, (size_t)n_valid, rocprim::plus<uint32_t>(), st));
    STAGE_LAUNCH(ctx, stats.launches, rgb_stats_kernel, 24.0 * n_valid, dim3(grid_of(n_valid, kRgBlock)), dim3(kRgBlock), 0, st, rank_of_pos, lab, segno, flag,
                 cloud->d_rgb, n_valid, seg_of_pos, stat, words);
    // 6. segment pairs: (seg u, seg v) -> min d2
    const size_t total = (size_t)n_valid * (size_t)k;
    STAGE_LAUNCH(ctx, stats.launches, rgb_pair_keys_kernel, 20.0 * total, dim3(grid_of(total, kRgBlock)), dim3(kRgBlock), 0, st, nbr, nd2, seg_of_pos, total, k,
                 pkey, pval);
    STAGE_PRIM(ctx, stats.launches, e, "rgb_sort_pairs", rocprim::radix_sort_pairs(d_tmp, (t1 = tb), pkey, pkey2, pval, pval2, total, 0, 64, st));
    STAGE_PRIM(ctx, stats.launches, e, "rgb_reduce_pairs",
               rocprim::reduce_by_key(d_tmp, (t1 = tb), pkey2, pval2, total, pkey, pval, words + 2, rocprim::minimum<uint32_t>(),
                                      rocprim::equal_to<unsigned long long>(), st));
    STAGE_LAUNCH(ctx, stats.launches, rgb_pair_count_kernel, 16.0, dim3(1), dim3(1), 0, st, pkey, words + 2, words);
    uint32_t hw[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(hw, words, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    ++stats.host_syncs;
    RGB_CHECK();
    S = hw[0];
    const uint32_t np = hw[1];
    if (S == 0 || S > n_valid || np > total) return set_err(ctx, OPE_ESTATE, std::string(who) + "inconsistent segment counts");
    // the kept tables: the first k of every segment by (d2, seg v).  (Launched for P = 0 too: the budget does not depend on P.)
    const size_t sk = (size_t)S * (size_t)k;
    auto *kept_d = (uint32_t *)tmp.get(4ull * sk, e), *kept_t = (uint32_t *)tmp.get(4ull * sk, e);
    if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
    const uint32_t np1 = std::max<uint32_t>(np, 1);
    STAGE_LAUNCH(ctx, stats.launches, rgb_pair_rekey_kernel, 24.0 * np, dim3(grid_of(np1, kRgBlock)), dim3(kRgBlock), 0, st, pkey, pval, np, pkey2, pval2);
    STAGE_PRIM(ctx, stats.launches, e, "rgb_sort_kept", rocprim::radix_sort_pairs(d_tmp, (t1 = tb), pkey2, pkey, pval2, pval, (size_t)np, 0, 32 + sbits, st));
    STAGE_LAUNCH(ctx, stats.launches, rgb_pair_start_kernel, 12.0 * np, dim3(grid_of(np1, kRgBlock)), dim3(kRgBlock), 0, st, pkey, np, pstart);
    STAGE_LAUNCH(ctx, stats.launches, rgb_pair_keep_kernel, 24.0 * np, dim3(grid_of(np1, kRgBlock)), dim3(kRgBlock), 0, st, pkey, pval, np, pstart, k, kept_d,
                 kept_t, kept_n);
    // 7. the one download of the tables, and the merges on the host
    Segments g;
    g.S = S;
    g.k = k;
    g.stat.resize(4ull * S);
    g.kept_d.resize(sk);
    g.kept_t.resize(sk);
    g.kept_n.resize(S);
    if (e == hipSuccess) e = hipMemcpyAsync(g.stat.data(), stat, 16ull * S, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(g.kept_n.data(), kept_n, 4ull * S, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(g.kept_d.data(), kept_d, 4ull * sk, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(g.kept_t.data(), kept_t, 4ull * sk, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    ++stats.host_syncs;
    RGB_CHECK();
    for (size_t s = 0; s < S; ++s) {
      if (g.stat[4 * s] == 0 || g.kept_n[s] > (uint32_t)k) return set_err(ctx, OPE_ESTATE, std::string(who) + "inconsistent segment tables");
      for (uint32_t q = 0; q < g.kept_n[s]; ++q)
        if (g.kept_t[s * k + q] >= S) return set_err(ctx, OPE_ESTATE, std::string(who) + "inconsistent segment tables");
    }
    stats.segments = (int64_t)S;
    stats.segment_pairs = (int64_t)np;
    merge_segments(g, d2_thr, r2_thr, (uint32_t)p.min_size, (uint32_t)p.max_size, cluster_of_seg, cluster_size, stats);
  }
  // 8. the upload (cluster of every segment, offsets), labels, the sort of the indices
  res.K = (uint32_t)cluster_size.size();
  res.kw = std::min<size_t>(res.K, kcap);
  std::vector<uint32_t> up(nv1 + kcap + 1, 0u);
  for (size_t s = 0; s < cluster_of_seg.size(); ++s) up[s] = (uint32_t)cluster_of_seg[s];
  uint32_t *off = up.data() + nv1;
  for (size_t q = 0; q < kcap; ++q) off[q + 1] = off[q] + (q < res.kw ? cluster_size[q] : 0u);
  uint32_t *roff = d_up + nv1;
  e = hipMemcpyAsync(d_up, up.data(), 4ull * up.size(), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  ++stats.host_syncs;
  RGB_CHECK();
  STAGE_LAUNCH(ctx, stats.launches, rgb_label_kernel, 32.0 * n, dim3(grid_of(n, kRgBlock)), dim3(kRgBlock), 0, st, pos_by_o, seg_of_pos, (const int32_t *)d_up,
               n, n_valid, (uint32_t)kcap, label, lkey, lval);
  STAGE_PRIM(ctx, stats.launches, e, "rgb_sort_labels", rocprim::radix_sort_pairs(d_tmp, (t1 = tb), lkey, lkey2, lval, idx, n, 0, lbits, st));
  if (e == hipSuccess && want_idx && n) e = hipMemcpyAsync(out_idx, idx, 4ull * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && out_label && n) e = hipMemcpyAsync(out_label, label, 4ull * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  ++stats.host_syncs;
  RGB_CHECK();
  stats.sweeps = sweeps;
  stats.one_way_edges = (int64_t)one_way;
  res.off.assign(off, off + res.kw + 1);
  if (out_offsets)
    for (size_t q = 0; q <= res.kw; ++q) out_offsets[q] = (int32_t)res.off[q];
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

void ope_region_rgb_default_params(ope_region_rgb_params *p) {
  if (!p) return;
  p->region_neighbour_number = 100;
  p->distance_threshold = 0.1;
  p->point_color_threshold = 10.0;
  p->region_color_threshold = 10.0;
  p->min_size = 700;
  p->max_size = INT32_MAX;
}

int ope_region_grow_rgb(ope_ctx *ctx, const ope_cloud *cloud, const ope_region_rgb_params *params, size_t max_clusters, size_t *n_clusters, int32_t *out_idx,
                        int32_t *out_offsets, int32_t *out_label) {
  static const char *who = "ope_region_grow_rgb: ";
  ope_region_rgb_params p;
  const int rc0 = check_params(ctx, who, cloud, params, n_clusters, p);
  if (rc0 != OPE_OK) return rc0;
  if (max_clusters > 0 && (!out_idx || !out_offsets)) return set_err(ctx, OPE_EINVAL, std::string(who) + "out_idx and out_offsets are required");
  *n_clusters = 0;
  if (cloud->n == 0) { if (out_offsets) out_offsets[0] = 0; return OPE_OK; }
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  TraceRange r(ctx, "region_grow_rgb");
  CallTmp tmp{ctx->stream, {}};
  Result res;
  const int32_t *d_idx; const uint32_t *d_roff, *d_pos; const float4 *d_pts;
  const int rc = region_rgb_core(ctx, tmp, who, cloud, p, max_clusters, max_clusters > 0, out_idx, out_offsets, out_label, res, &d_idx, &d_roff, &d_pts,
                                 &d_pos);
  if (rc != OPE_OK) return rc;
  *n_clusters = res.K;
  return OPE_OK;
}

int ope_region_grow_rgb_cloud(ope_ctx *ctx, const ope_cloud *cloud, const ope_region_rgb_params *params, size_t max_clusters, size_t *n_clusters,
                              ope_cloud **out_clouds, int32_t *out_idx, int32_t *out_offsets) {
  static const char *who = "ope_region_grow_rgb_cloud: ";
  ope_region_rgb_params p;
  const int rc0 = check_params(ctx, who, cloud, params, n_clusters, p);
  if (rc0 != OPE_OK) return rc0;
  if (max_clusters > 0 && !out_clouds) return set_err(ctx, OPE_EINVAL, std::string(who) + "out_clouds is required");
  *n_clusters = 0;
  if (cloud->n == 0) {
    for (size_t q = 0; q < max_clusters; ++q) out_clouds[q] = nullptr;
    if (out_offsets) out_offsets[0] = 0;
    return OPE_OK;
  }
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  TraceRange r(ctx, "region_grow_rgb");
  CallTmp tmp{ctx->stream, {}};
  Result res;
  const int32_t *d_idx; const uint32_t *d_roff, *d_pos; const float4 *d_pts;
  int rc = region_rgb_core(ctx, tmp, who, cloud, p, max_clusters, out_idx != nullptr, out_idx, out_offsets, nullptr, res, &d_idx, &d_roff, &d_pts, &d_pos);
  if (rc != OPE_OK) return rc;
  for (size_t q = 0; q < max_clusters; ++q) out_clouds[q] = nullptr;
  if (res.kw > 0) {
    rc = clusters_build_clouds(ctx, tmp, who, cloud, res.kw, res.off, d_idx, d_roff, d_pts, d_pos, out_clouds, &ctx->region_rgb_stats.launches,
                               &ctx->region_rgb_stats.host_syncs);
    if (rc != OPE_OK) return rc;
  }
  *n_clusters = res.K;
  return OPE_OK;
}

int ope_region_rgb_last_stats(const ope_ctx *ctx, ope_region_rgb_stats *out) {
  if (!ctx || !out) return OPE_EINVAL;
  *out = ctx->region_rgb_stats;
  return OPE_OK;
}

}  // extern "C"
