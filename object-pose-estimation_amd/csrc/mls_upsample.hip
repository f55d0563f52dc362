// mls_upsample.hip — pcl::MovingLeastSquares::process with upsampling VOXEL_GRID_DILATION (RegMeshPcd::generateMesh,
// BuildModel/src/regmeshpcd.cpp:275-292; surface/include/pcl/surface/impl/mls.hpp: MLSVoxelGrid, performUpsampling,
// projectPointToMLSSurface), on the device.
//
//   mls_fit_records (mls.hip)   the two walks of moving least squares in record mode: the MLSResult of every point with 3 or more
//                               neighbours under its original index, orders 0 to 4; nothing moves.
//   mls_voxel_key_kernel        the 64-bit key of every finite point's voxel, with the point's original index beside it; rocPRIM
//                               radix sort + unique give the grid in ascending key order (std::map's order).
//   mls_voxel_dilate_kernel     one dilation round: 27 keys per voxel (out-of-range neighbours become a sentinel that sorts last
//                               and is dropped), then sort + unique again.  The host waits once per round for the count.
//   mls_project_kernel          one lane per voxel in key order: the voxel's position, a 1-nearest walk of the cloud's own tree
//                               from the leaf of the point carried with the key (ties to the lowest original index), the
//                               projection on that point's MLS surface, the keep rule, a flag.
//   rocPRIM scan of the flags, mls_upsample_scatter_kernel: the survivors in key order with their indices, normals, curvature
//                               and the colour word of their nearest point, in one launch.
// The sequence of launches and waits is fixed by the parameters (dilation_iterations, whether the cloud has colours), never by
// the points.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "bvh_traverse.hpp"
#include "mls_shared.hpp"

namespace ope {

constexpr int kUpBlock = 256;
constexpr unsigned long long kNoKey = ~0ull;              // a dropped dilation neighbour: sorts behind every key
constexpr unsigned long long kMaxDataSize = 1ull << 21;   // keys stay below 2^63
// words of the upsampling's own counters
enum { kUpValid = 0, kUpInvalidNearest = 1, kUpPolynomial = 2, kUpRejected = 3, kUpWords = 4 };

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// MLSVoxelGrid::getIndexIn3D; data_size 0 (every point within 2/3 of a voxel) decodes to cell (0, 0, 0)
__device__ __forceinline__ void mls_voxel_cell(unsigned long long key, unsigned long long ds, unsigned long long (&c)[3]) {
  if (ds == 0ull) { c[0] = c[1] = c[2] = 0ull; return; }
  c[0] = key / (ds * ds);
  const unsigned long long rem = key - c[0] * ds * ds;
  c[1] = rem / ds;
  c[2] = rem - c[1] * ds;
}

// MLSVoxelGrid's constructor: cell = int ((p - bmin) / voxel_size), float subtract, float divide, truncate; also counts the valid
// records (points with 3 or more neighbours)
__global__ __launch_bounds__(kUpBlock) void mls_voxel_key_kernel(CloudView c, float bx, float by, float bz, float vs, unsigned long long ds,
                                                                  const uint32_t *__restrict__ flag_orig, unsigned long long *__restrict__ keys,
                                                                  uint32_t *__restrict__ src, uint32_t *__restrict__ counters) {
  const uint32_t i = blockIdx.x * kUpBlock + threadIdx.x;
  uint32_t valid = 0;
  if (i < c.n_valid) {
    const float4 p = c.xyzw[i];
    const uint32_t orig = (uint32_t)__float_as_int(p.w);
    const unsigned long long c0 = (unsigned long long)(int)__fdiv_rn(__fsub_rn(p.x, bx), vs);
    const unsigned long long c1 = (unsigned long long)(int)__fdiv_rn(__fsub_rn(p.y, by), vs);
    const unsigned long long c2 = (unsigned long long)(int)__fdiv_rn(__fsub_rn(p.z, bz), vs);
    keys[i] = (c0 * ds + c1) * ds + c2;
    src[i] = orig;
    valid = flag_orig[orig];
  }
  valid = wave_sum_u32(valid);
  if ((threadIdx.x & 63u) == 0 && valid) atomicAdd(counters + kUpValid, valid);
}

// one dilation round: entry 27 t + r is neighbour r of voxel t (itself included), or kNoKey when a component leaves [0, data_size)
__global__ __launch_bounds__(kUpBlock) void mls_voxel_dilate_kernel(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ src,
                                                                     uint32_t n_vox, unsigned long long ds, unsigned long long *__restrict__ out_keys,
                                                                     uint32_t *__restrict__ out_src) {
  const size_t e = (size_t)blockIdx.x * kUpBlock + threadIdx.x;
  if (e >= (size_t)n_vox * 27u) return;
  const uint32_t t = (uint32_t)(e / 27u), r = (uint32_t)(e % 27u);
  unsigned long long c[3];
  mls_voxel_cell(keys[t], ds, c);
  const long long a0 = (long long)c[0] + (long long)(r / 9u) - 1, a1 = (long long)c[1] + (long long)((r / 3u) % 3u) - 1,
                  a2 = (long long)c[2] + (long long)(r % 3u) - 1;
  const long long lim = (long long)ds;
  const bool in = a0 >= 0 && a0 < lim && a1 >= 0 && a1 < lim && a2 >= 0 && a2 < lim;
  out_keys[e] = in ? ((unsigned long long)a0 * ds + (unsigned long long)a1) * ds + (unsigned long long)a2 : kNoKey;
  out_src[e] = src[t];
}

// the sentinel, if any neighbour was dropped, is the last distinct key: it does not count
__global__ void mls_voxel_count_kernel(const unsigned long long *__restrict__ keys, uint32_t *__restrict__ count) {
  if (threadIdx.x == 0 && blockIdx.x == 0 && *count > 0u && keys[*count - 1u] == kNoKey) *count -= 1u;
}

// 1-nearest with FLANN's implementation-defined choice among equal distances replaced by a rule that does not depend on the tree:
// the lowest ORIGINAL index.  Subtrees whose bound EQUALS the best distance are still entered.
struct NearestLowestIndexVisitor {
  float best;
  uint32_t pos, orig;
  __device__ __forceinline__ bool prune(float bound) const { return bound > best; }
  __device__ __forceinline__ void point(float d, const v4f &p, uint32_t i, uint32_t) {
    const uint32_t o = (uint32_t)__float_as_int(p.w);
    if (d < best || (d == best && o < orig)) { best = d; pos = i; orig = o; }
  }
  __device__ __forceinline__ void on_node() {}
};

__device__ __forceinline__ float dot3_f32(const float (&a)[3], const float (&b)[3]) {
  return __fadd_rn(__fadd_rn(__fmul_rn(a[0], b[0]), __fmul_rn(a[1], b[1])), __fmul_rn(a[2], b[2]));
}

// performUpsampling's VOXEL_GRID_DILATION loop body and projectPointToMLSSurface, one lane per voxel in key order
__global__ __launch_bounds__(kUpBlock) void mls_project_kernel(BvhView tgt, const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ src,
                                                                uint32_t n_vox, unsigned long long ds, float bx, float by, float bz, float vs,
                                                                int order, int compute_normals, const uint32_t *__restrict__ self_leaf,
                                                                const uint32_t *__restrict__ flag_orig, const MlsRecord *__restrict__ rec,
                                                                float *__restrict__ pos_out, float4 *__restrict__ nrm_out,
                                                                int32_t *__restrict__ near_out, uint32_t *__restrict__ keep,
                                                                uint32_t *__restrict__ counters) {
  __shared__ float s_stk[kMaxDepth + 1][kUpBlock];
  float *stk = &s_stk[0][threadIdx.x];
  const uint32_t t = blockIdx.x * kUpBlock + threadIdx.x;
  uint32_t n_invalid = 0, n_poly = 0, n_rejected = 0;
  if (t < n_vox) {
    unsigned long long cell[3];
    mls_voxel_cell(keys[t], ds, cell);
    // MLSVoxelGrid::getPosition: a float multiply, then a float add
    const float pos[3] = {__fadd_rn(__fmul_rn((float)cell[0], vs), bx), __fadd_rn(__fmul_rn((float)cell[1], vs), by),
                          __fadd_rn(__fmul_rn((float)cell[2], vs), bz)};
    NearestLowestIndexVisitor v{INFINITY, kNoPos, 0xffffffffu};
    bvh_traverse(tgt, pos[0], pos[1], pos[2], v, stk, kUpBlock, self_leaf[src[t]]);
    const uint32_t j = v.orig;
    uint32_t kept = 0;
    near_out[t] = (int32_t)j;
    if (v.pos == kNoPos || !flag_orig[j]) {
      ++n_invalid;
    } else {
      const v4f qp = ld16(tgt.pts + v.pos);
      const float q[3] = {qp.x, qp.y, qp.z};
      const MlsRecord *r = rec + j;
      const double mean[3] = {r->mean[0], r->mean[1], r->mean[2]}, n[3] = {r->n[0], r->n[1], r->n[2]};
      const uint32_t flags = r->flags;
      double u[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0};   // 1.7 leaves the axes zero below nr_coeff neighbours
      if (flags & kMlsRecAxes) mls_axes(n[0], n[1], n[2], u, w);
      const float uf[3] = {(float)u[0], (float)u[1], (float)u[2]}, wf[3] = {(float)w[0], (float)w[1], (float)w[2]};
      const float dd[3] = {__fsub_rn(pos[0], q[0]), __fsub_rn(pos[1], q[1]), __fsub_rn(pos[2], q[2])};
      const float u_disp = dot3_f32(dd, uf), v_disp = dot3_f32(dd, wf);
      const int nr = (order + 1) * (order + 2) / 2;
      double n_disp = 0.0, d_u = 0.0, d_v = 0.0;
      if ((flags & kMlsRecAxes) && (flags & kMlsRecSolved) && r->m >= 5 * nr && isfinite(r->c[0])) {
        ++n_poly;
        int k = 0;
        float u_pow = 1.f, u_pow_prev = 1.f;
        for (int ui = 0; ui <= order; ++ui) {
          float v_pow = 1.f, v_pow_prev = 1.f;
          for (int vi = 0; vi <= order - ui; ++vi) {
            const double c = r->c[k++];
            n_disp += (double)__fmul_rn(u_pow, v_pow) * c;
            if (ui >= 1) d_u += c * ((double)ui * (double)__fmul_rn(u_pow_prev, v_pow));
            if (vi >= 1) d_v += c * ((double)vi * (double)__fmul_rn(u_pow, v_pow_prev));
            v_pow_prev = v_pow;
            v_pow = __fmul_rn(v_pow, v_disp);
          }
          u_pow_prev = u_pow;
          u_pow = __fmul_rn(u_pow, u_disp);
        }
      }
      float res[3], nrm[3];
      double nd[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        res[a] = (float)(((mean[a] + u[a] * (double)u_disp) + w[a] * (double)v_disp) + n[a] * n_disp);
        nd[a] = (n[a] - d_u * u[a]) - d_v * w[a];
      }
      const double len = sqrt((nd[0] * nd[0] + nd[1] * nd[1]) + nd[2] * nd[2]);
#pragma unroll
      for (int a = 0; a < 3; ++a) nrm[a] = compute_normals ? (float)(nd[a] / len) : (float)n[a];
      const float da[3] = {__fsub_rn(res[0], q[0]), __fsub_rn(res[1], q[1]), __fsub_rn(res[2], q[2])};
      const float d_before = __fsqrt_rn(dot3_f32(dd, dd)), d_after = __fsqrt_rn(dot3_f32(da, da));
      if (d_after > d_before) {
        ++n_rejected;
      } else {
        kept = 1u;
        pos_out[3 * (size_t)t] = res[0]; pos_out[3 * (size_t)t + 1] = res[1]; pos_out[3 * (size_t)t + 2] = res[2];
        nrm_out[t] = make_float4(nrm[0], nrm[1], nrm[2], r->curvature);
      }
    }
    keep[t] = kept;
  }
  n_invalid = wave_sum_u32(n_invalid); n_poly = wave_sum_u32(n_poly); n_rejected = wave_sum_u32(n_rejected);
  if ((threadIdx.x & 63u) == 0) {
    if (n_invalid) atomicAdd(counters + kUpInvalidNearest, n_invalid);
    if (n_poly) atomicAdd(counters + kUpPolynomial, n_poly);
    if (n_rejected) atomicAdd(counters + kUpRejected, n_rejected);
  }
}

// sorted position of every original index (the colour words lie in the cloud's sorted order)
__global__ __launch_bounds__(256) void mls_upsample_inverse_kernel(CloudView c, uint32_t *__restrict__ pos_of_orig) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p < c.n) pos_of_orig[(uint32_t)__float_as_int(c.xyzw[p].w)] = p;
}

// the survivors in key order: point, normal + curvature, index of the nearest input point, and its colour word in the same launch
__global__ __launch_bounds__(256) void mls_upsample_scatter_kernel(uint32_t n_vox, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ rank,
                                                                    const float *__restrict__ pos_vox, const float4 *__restrict__ nrm_vox,
                                                                    const int32_t *__restrict__ near_vox, const uint32_t *__restrict__ pos_of_orig,
                                                                    const uint32_t *__restrict__ rgb_in, float *__restrict__ raw,
                                                                    float4 *__restrict__ nrm_out, int32_t *__restrict__ idx_out,
                                                                    uint32_t *__restrict__ rgb_raw) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_vox || !keep[t]) return;
  const uint32_t dst = rank[t];
  raw[3 * (size_t)dst] = pos_vox[3 * (size_t)t]; raw[3 * (size_t)dst + 1] = pos_vox[3 * (size_t)t + 1]; raw[3 * (size_t)dst + 2] = pos_vox[3 * (size_t)t + 2];
  nrm_out[dst] = nrm_vox[t];
  idx_out[dst] = near_vox[t];
  if (rgb_raw) rgb_raw[dst] = rgb_in[pos_of_orig[(uint32_t)near_vox[t]]];
}

// what a call leaves on the device (temporaries of the context's stream; upsample_release gives them back)
struct UpsampleOut {
  float *d_raw = nullptr;        // count * 3, key order
  float4 *d_nrm = nullptr;       // count: normal, curvature
  int32_t *d_idx = nullptr;      // count
  uint32_t *d_rgb_raw = nullptr; // count, when the input has colours
  size_t count = 0;
  uint32_t n_finite = 0;
  float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
};

static void upsample_release(ope_ctx *ctx, UpsampleOut &o) {
  for (void *p : {(void *)o.d_raw, (void *)o.d_nrm, (void *)o.d_idx, (void *)o.d_rgb_raw}) tmp_free(ctx->stream, p);
  o = UpsampleOut();
}

// MLSVoxelGrid: data_size = uint64 (1.5 * max extent / voxel_size), the extent a float difference
static bool upsample_data_size(const ope_cloud *cloud, float voxel_size, unsigned long long *ds) {
  float ext = 0.f;
  for (int d = 0; d < 3; ++d) ext = std::max(ext, cloud->bb_hi[d] - cloud->bb_lo[d]);
  const double v = 1.5 * (double)ext / (double)voxel_size;
  if (!(v < (double)kMaxDataSize + 1.0)) return false;
  *ds = (unsigned long long)v;
  return *ds <= kMaxDataSize;
}

static int upsample_check(ope_ctx *ctx, const ope_cloud *cloud, const ope_mls_upsample_params *p, const char *who) {
  if (!ctx || !cloud || !p) return set_err(ctx, OPE_EINVAL, std::string(who) + ": bad argument");
  if (!(p->radius > 0) || !std::isfinite(p->radius) || !((float)p->radius * (float)p->radius > 0.f))
    return set_err(ctx, OPE_EINVAL, std::string(who) + ": the radius must be positive");
  if (p->order < 0 || p->order > kMlsMaxOrder) return set_err(ctx, OPE_EINVAL, std::string(who) + ": polynomial orders 0 to 4 are supported");
  if (!(p->sqr_gauss_param >= 0) || !std::isfinite(p->sqr_gauss_param))
    return set_err(ctx, OPE_EINVAL, std::string(who) + ": sqr_gauss_param must be positive, or 0 for radius^2");
  if (!(p->voxel_size > 0.f) || !std::isfinite(p->voxel_size)) return set_err(ctx, OPE_EINVAL, std::string(who) + ": voxel_size must be positive");
  if (p->dilation_iterations < 0 || p->dilation_iterations > 8)
    return set_err(ctx, OPE_EINVAL, std::string(who) + ": dilation_iterations must be 0 to 8");
  if (cloud->n > (size_t)0x7fffffff) return set_err(ctx, OPE_EINVAL, std::string(who) + ": more than 2^31-1 points");
  unsigned long long ds = 0;
  if (cloud->n_valid && !upsample_data_size(cloud, p->voxel_size, &ds))
    return set_err(ctx, OPE_EINVAL, std::string(who) + ": the voxel grid would be more than 2^21 voxels wide");
  return OPE_OK;
}

// sort (keys, src) of `size` entries from buffer 0 into buffer 1, keep the first entry of every distinct key back in buffer 0, count
// them in d_count and take the sentinel off the count: three rocPRIM calls and a launch
static hipError_t upsample_sort_unique(hipStream_t s, unsigned long long *const k[2], uint32_t *const v[2], size_t size, uint32_t *d_count,
                                       void *d_tmp, size_t tmp_bytes) {
  size_t tb = tmp_bytes;
  hipError_t e = rocprim::radix_sort_pairs(d_tmp, tb, k[0], k[1], v[0], v[1], size, 0u, 64u, s);
  tb = tmp_bytes;
  if (e == hipSuccess) e = rocprim::unique_by_key(d_tmp, tb, k[1], v[1], k[0], v[0], d_count, size, rocprim::equal_to<unsigned long long>(), s);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(mls_voxel_count_kernel, dim3(1), dim3(64), 0, s, k[0], d_count);
    e = hipGetLastError();
  }
  return e;
}
static hipError_t upsample_sort_unique_bytes(hipStream_t s, size_t size, size_t *bytes) {
  size_t a = 0, b = 0;
  unsigned long long *k = nullptr;
  uint32_t *v = nullptr;
  hipError_t e = rocprim::radix_sort_pairs(nullptr, a, k, k, v, v, size, 0u, 64u, s);
  if (e == hipSuccess) e = rocprim::unique_by_key(nullptr, b, k, v, k, v, v, size, rocprim::equal_to<unsigned long long>(), s);
  *bytes = std::max<size_t>(std::max(a, b), 16);
  return e;
}

static int upsample_core(ope_ctx *ctx, const ope_cloud *cloud, const ope_mls_upsample_params &p, UpsampleOut &o, const char *who) {
  const size_t n = cloud->n, nv = cloud->n_valid;
  ope_mls_upsample_stats &st = ctx->mls_upsample_stats;
  st = ope_mls_upsample_stats{};
  st.n_in = (int64_t)n;
  if (nv == 0) return OPE_OK;
  unsigned long long ds = 0;
  upsample_data_size(cloud, p.voxel_size, &ds);   // (checked by upsample_check)
  st.data_size = (int64_t)ds;
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  TraceRange r(ctx, "mls_upsample");
  ope_index *ix = nullptr;
  ope_index_params ip;
  ope_index_default_params(&ip);
  ip.grid = 0;   // the index serves the walks of this call
  int rc = index_build_tmp(ctx, cloud, &ip, &ix);
  if (rc != OPE_OK) return rc;
  st.launches += 1;   // the index build, booked as one
  const float bx = cloud->bb_lo[0], by = cloud->bb_lo[1], bz = cloud->bb_lo[2], vs = p.voxel_size;
  uint32_t *d_self = nullptr, *d_flag = nullptr, *d_stats = nullptr, *d_counters = nullptr, *d_count = nullptr, *d_inv = nullptr;
  uint32_t *d_keep = nullptr, *d_rank = nullptr;
  MlsRecord *d_rec = nullptr;
  unsigned long long *d_k[2] = {nullptr, nullptr};
  uint32_t *d_v[2] = {nullptr, nullptr};
  float *d_pos = nullptr;
  float4 *d_nrm = nullptr;
  int32_t *d_near = nullptr;
  void *d_tmp = nullptr;
  uint32_t init[kMlsWords] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, res[kMlsWords], counters[kUpWords] = {0, 0, 0, 0};
  uint32_t n_vox = 0, count = 0;
  bool too_many = false;
  hipError_t e = tmp_malloc(s, (void **)&d_self, 4 * n);
  if (e == hipSuccess) e = tmp_malloc(s, (void **)&d_flag, 4 * (n + 1));
  if (e == hipSuccess) e = tmp_malloc(s, (void **)&d_stats, sizeof init);
  if (e == hipSuccess) e = tmp_malloc(s, (void **)&d_counters, sizeof counters + 4);
  if (e == hipSuccess) e = tmp_malloc(s, (void **)&d_rec, sizeof(MlsRecord) * n);
  for (int b = 0; b < 2; ++b) {
    if (e == hipSuccess) e = tmp_malloc(s, (void **)&d_k[b], 8 * nv);
    if (e == hipSuccess) e = tmp_malloc(s, (void **)&d_v[b], 4 * nv);
  }
  if (e == hipSuccess && cloud->d_rgb) e = tmp_malloc(s, (void **)&d_inv, 4 * n);
  if (e == hipSuccess) {
    d_count = d_counters + kUpWords;
    e = self_leaves(s, ix->view(), n, d_self);
    st.launches += 2;
  }
  if (e == hipSuccess) { e = hipMemsetAsync(d_flag, 0, 4 * (n + 1), s); st.launches += 1; }
  if (e == hipSuccess) { e = h2d_copy(s, d_stats, init, sizeof init); st.launches += 1; }
  if (e == hipSuccess) { e = hipMemsetAsync(d_counters, 0, sizeof counters + 4, s); st.launches += 1; }
  if (e == hipSuccess) {
    const float r2 = (float)p.radius * (float)p.radius;
    const double sgp = p.sqr_gauss_param != 0.0 ? p.sqr_gauss_param : p.radius * p.radius;   // setSearchRadius: sqr_gauss_param_ = radius^2
    e = mls_fit_records(ctx, cloud, ix, d_self, r2, sgp, p.polynomial_fit, p.order, d_flag, d_rec, d_stats);
    st.launches += 2;
  }
  // ---- the grid: keys of the points, sorted and made distinct
  if (e == hipSuccess) {
    KernelTimer kt(ctx, "mls_voxel_key_kernel", 28.0 * (double)nv);
    hipLaunchKernelGGL(mls_voxel_key_kernel, dim3((unsigned)((nv + kUpBlock - 1) / kUpBlock)), dim3(kUpBlock), 0, s, cloud->view(), bx, by, bz, vs, ds,
                       d_flag, d_k[0], d_v[0], d_counters);
    kt.stop();
    e = hipGetLastError();
    st.launches += 1;
  }
  size_t tb = 0;
  if (e == hipSuccess) e = upsample_sort_unique_bytes(s, nv, &tb);
  if (e == hipSuccess) e = tmp_malloc(s, &d_tmp, tb);
  if (e == hipSuccess) { e = upsample_sort_unique(s, d_k, d_v, nv, d_count, d_tmp, tb); st.launches += 3; }
  if (e == hipSuccess) { e = hipMemcpyAsync(&n_vox, d_count, 4, hipMemcpyDeviceToHost, s); st.launches += 1; }
  if (e == hipSuccess) { e = hipStreamSynchronize(s); st.host_syncs += 1; }
  tmp_free(s, d_tmp);
  d_tmp = nullptr;
  // ---- dilation rounds: 27 keys per voxel, sorted and made distinct; one wait per round for the count
  for (int round = 0; e == hipSuccess && round < p.dilation_iterations && !too_many; ++round) {
    const size_t m = (size_t)n_vox * 27;
    if (m > (size_t)0x7fffffff) { too_many = true; break; }
    unsigned long long *nk[2] = {nullptr, nullptr};
    uint32_t *nvl[2] = {nullptr, nullptr};
    for (int b = 0; b < 2; ++b) {
      if (e == hipSuccess) e = tmp_malloc(s, (void **)&nk[b], 8 * std::max<size_t>(m, 1));
      if (e == hipSuccess) e = tmp_malloc(s, (void **)&nvl[b], 4 * std::max<size_t>(m, 1));
    }
    if (e == hipSuccess && m) {
      KernelTimer kt(ctx, "mls_voxel_dilate_kernel", 12.0 * (double)n_vox + 12.0 * (double)m);
      hipLaunchKernelGGL(mls_voxel_dilate_kernel, dim3((unsigned)((m + kUpBlock - 1) / kUpBlock)), dim3(kUpBlock), 0, s, d_k[0], d_v[0], n_vox, ds, nk[0],
                         nvl[0]);
      kt.stop();
      e = hipGetLastError();
    }
    if (e == hipSuccess && m) e = upsample_sort_unique_bytes(s, m, &tb);
    if (e == hipSuccess && m) e = tmp_malloc(s, &d_tmp, tb);
    if (e == hipSuccess && m) e = upsample_sort_unique(s, nk, nvl, m, d_count, d_tmp, tb);
    if (e == hipSuccess && m) e = hipMemcpyAsync(&n_vox, d_count, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    st.launches += 5;   // booked for an empty grid too, which dilates to nothing
    st.host_syncs += 1;
    tmp_free(s, d_tmp);
    d_tmp = nullptr;
    for (int b = 0; b < 2; ++b) {
      tmp_free(s, d_k[b]); tmp_free(s, d_v[b]);
      d_k[b] = nk[b]; d_v[b] = nvl[b];
    }
  }
  // ---- one lane per voxel: nearest point, projection, keep rule; then the ranks of the survivors
  const size_t nx = std::max<size_t>(n_vox, 1);
  if (e == hipSuccess && !too_many) {
    e = tmp_malloc(s, (void **)&d_keep, 4 * (nx + 1));
    if (e == hipSuccess) e = tmp_malloc(s, (void **)&d_rank, 4 * (nx + 1));
    if (e == hipSuccess) e = tmp_malloc(s, (void **)&d_pos, 12 * nx);
    if (e == hipSuccess) e = tmp_malloc(s, (void **)&d_nrm, 16 * nx);
    if (e == hipSuccess) e = tmp_malloc(s, (void **)&d_near, 4 * nx);
    if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, tb, d_keep, d_rank, 0u, nx + 1, rocprim::plus<uint32_t>(), s);
    if (e == hipSuccess) e = tmp_malloc(s, &d_tmp, std::max<size_t>(tb, 16));
    if (e == hipSuccess) e = hipMemsetAsync(d_keep, 0, 4 * (nx + 1), s);
    if (e == hipSuccess && n_vox) {
      // algorithmic bytes: key, carried index and its leaf (16), the nearest point and its record (16 + 184), the outputs (36)
      KernelTimer kt(ctx, "mls_project_kernel", 252.0 * (double)n_vox);
      hipLaunchKernelGGL(mls_project_kernel, dim3((n_vox + kUpBlock - 1) / kUpBlock), dim3(kUpBlock), 0, s, ix->view(), d_k[0], d_v[0], n_vox, ds, bx, by, bz,
                         vs, p.order, p.compute_normals, d_self, d_flag, d_rec, d_pos, d_nrm, d_near, d_keep, d_counters);
      kt.stop();
      e = hipGetLastError();
    }
    if (e == hipSuccess && n_vox) e = mls_bbox(s, d_pos, d_keep, n_vox, d_stats);
    size_t t1 = std::max<size_t>(tb, 16);
    if (e == hipSuccess) e = rocprim::exclusive_scan(d_tmp, t1, d_keep, d_rank, 0u, nx + 1, rocprim::plus<uint32_t>(), s);
    if (e == hipSuccess) e = hipMemcpyAsync(&count, d_rank + nx, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(res, d_stats, sizeof res, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(counters, d_counters, sizeof counters, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // the wait for what the host needs: count, bounding box, statistics
    st.launches += 7;
    st.host_syncs += 1;
  }
  if (e == hipSuccess && !too_many) {
    if (cloud->d_rgb) {
      hipLaunchKernelGGL(mls_upsample_inverse_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, cloud->view(), d_inv);
      e = hipGetLastError();
      st.launches += 1;
    }
    st.launches += 1;   // the scatter, booked for an empty result too
    if (e == hipSuccess && count) {
      e = tmp_malloc(s, (void **)&o.d_raw, 12 * (size_t)count);
      if (e == hipSuccess) e = tmp_malloc(s, (void **)&o.d_nrm, 16 * (size_t)count);
      if (e == hipSuccess) e = tmp_malloc(s, (void **)&o.d_idx, 4 * (size_t)count);
      if (e == hipSuccess && cloud->d_rgb) e = tmp_malloc(s, (void **)&o.d_rgb_raw, 4 * (size_t)count);
      if (e == hipSuccess) {
        hipLaunchKernelGGL(mls_upsample_scatter_kernel, dim3((n_vox + 255) / 256), dim3(256), 0, s, n_vox, d_keep, d_rank, d_pos, d_nrm, d_near, d_inv,
                           (const uint32_t *)cloud->d_rgb, o.d_raw, o.d_nrm, o.d_idx, o.d_rgb_raw);
        e = hipGetLastError();
      }
    }
  }
  for (void *q : {(void *)d_self, (void *)d_flag, (void *)d_stats, (void *)d_counters, (void *)d_inv, (void *)d_keep, (void *)d_rank, (void *)d_rec,
                  (void *)d_k[0], (void *)d_k[1], (void *)d_v[0], (void *)d_v[1], (void *)d_pos, (void *)d_nrm, (void *)d_near, d_tmp})
    tmp_free(s, q);
  ope_index_free(ix);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(s);   // (no copy into this frame may outlive it)
    upsample_release(ctx, o);
    return set_err(ctx, OPE_EHIP, std::string(who) + ": " + hipGetErrorString(e));
  }
  if (too_many) {
    (void)hipStreamSynchronize(s);
    return set_err(ctx, OPE_EINVAL, std::string(who) + ": a dilation round would make more than 2^31-1 candidate voxels");
  }
  auto unkey = [](uint32_t k) { const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; float f; std::memcpy(&f, &u, 4); return f; };
  o.count = count;
  o.n_finite = res[kMlsFinite];
  if (o.n_finite > 0)
    for (int d = 0; d < 3; ++d) { o.lo[d] = unkey(res[kMlsMin + d]); o.hi[d] = unkey(res[kMlsMax + d]); }
  st.n_valid = (int64_t)counters[kUpValid];
  st.n_voxels = (int64_t)n_vox;
  st.n_invalid_nearest = (int64_t)counters[kUpInvalidNearest];
  st.n_polynomial = (int64_t)counters[kUpPolynomial];
  st.n_rejected_farther = (int64_t)counters[kUpRejected];
  st.n_out = (int64_t)count;
  return OPE_OK;
}

}  // namespace ope

using namespace ope;

extern "C" void ope_mls_upsample_default_params(ope_mls_upsample_params *p) {
  if (!p) return;
  p->radius = 0.0;              // MovingLeastSquares: search_radius_ (0); generateMesh passes 0.03 (regmeshpcd.cpp:285)
  p->polynomial_fit = 1;        // regmeshpcd.cpp:283: setPolynomialFit (true)
  p->order = 2;                 // MovingLeastSquares: order_ (2); generateMesh passes 4
  p->sqr_gauss_param = 0.0;     // 0: radius^2, as setSearchRadius sets it
  p->compute_normals = 0;       // MovingLeastSquares: compute_normals_ (false)
  p->voxel_size = 1.0f;         // MovingLeastSquares: voxel_size_ (1.0); generateMesh passes 0.002
  p->dilation_iterations = 0;   // MovingLeastSquares: dilation_iteration_num_ (0)
}

extern "C" int ope_mls_upsample(ope_ctx *ctx, const ope_cloud *cloud, const ope_mls_upsample_params *params, float *out_xyz, float *out_normals,
                                float *out_curvature, int32_t *out_idx, size_t capacity, size_t *n_out) {
  if (n_out) *n_out = 0;
  if (!n_out) return set_err(ctx, OPE_EINVAL, "ope_mls_upsample: bad argument");
  int rc = upsample_check(ctx, cloud, params, "ope_mls_upsample");
  if (rc != OPE_OK) return rc;
  UpsampleOut o;
  rc = upsample_core(ctx, cloud, *params, o, "ope_mls_upsample");
  if (rc != OPE_OK) return rc;
  const size_t m = o.count;
  if (m > capacity && (out_xyz || out_normals || out_curvature || out_idx)) {
    upsample_release(ctx, o);
    *n_out = m;
    return set_err(ctx, OPE_EINVAL, "ope_mls_upsample: capacity is too small for the result (*n_out holds the size it needs)");
  }
  hipError_t e = hipSuccess;
  if (m) {
    std::vector<float> nrm;
    if (out_normals || out_curvature) nrm.resize(4 * m);
    if (out_xyz) e = hipMemcpyAsync(out_xyz, o.d_raw, 12 * m, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && out_idx) e = hipMemcpyAsync(out_idx, o.d_idx, 4 * m, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && !nrm.empty()) e = hipMemcpyAsync(nrm.data(), o.d_nrm, 16 * m, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = e2;
    if (e == hipSuccess && !nrm.empty())
      for (size_t i = 0; i < m; ++i) {
        if (out_normals) { out_normals[3 * i] = nrm[4 * i]; out_normals[3 * i + 1] = nrm[4 * i + 1]; out_normals[3 * i + 2] = nrm[4 * i + 2]; }
        if (out_curvature) out_curvature[i] = nrm[4 * i + 3];
      }
  }
  ctx->mls_upsample_stats.launches += 3;   // the copies to the caller's arrays, booked whether asked for or not
  ctx->mls_upsample_stats.host_syncs += 1;
  upsample_release(ctx, o);
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string("ope_mls_upsample: ") + hipGetErrorString(e));
  *n_out = m;
  return OPE_OK;
}

extern "C" int ope_mls_upsample_cloud(ope_ctx *ctx, const ope_cloud *cloud, const ope_mls_upsample_params *params, ope_cloud **out,
                                      int32_t *out_idx, size_t capacity, size_t *n_out) {
  if (out) *out = nullptr;
  if (n_out) *n_out = 0;
  if (!out || !n_out) return set_err(ctx, OPE_EINVAL, "ope_mls_upsample_cloud: bad argument");
  int rc = upsample_check(ctx, cloud, params, "ope_mls_upsample_cloud");
  if (rc != OPE_OK) return rc;
  UpsampleOut o;
  rc = upsample_core(ctx, cloud, *params, o, "ope_mls_upsample_cloud");
  if (rc != OPE_OK) return rc;
  const size_t m = o.count;
  if (out_idx && m > capacity) {
    upsample_release(ctx, o);
    *n_out = m;
    return set_err(ctx, OPE_EINVAL, "ope_mls_upsample_cloud: capacity is too small for out_idx (*n_out holds the size it needs)");
  }
  ctx->mls_upsample_stats.launches += 5;   // the Morton ordering (3), the normals' gather and the copy of out_idx, booked whether needed or not
  ctx->mls_upsample_stats.host_syncs += 2; // the Morton ordering's own, and the end of the call
  if (m == 0) {
    // an empty cloud, coloured if the input was (and with the normals' buffer when they were asked for)
    OPE_HIP(ctx, hipSetDevice(ctx->device));
    rc = select_cloud_device(ctx, cloud, nullptr, 0, out);
    if (rc == OPE_OK && params->compute_normals && !(*out)->d_nrm) {
      const hipError_t e = hipMalloc((void **)&(*out)->d_nrm, sizeof(float4));
      if (e != hipSuccess) { ope_cloud_free(*out); *out = nullptr; return set_err(ctx, OPE_EHIP, std::string("ope_mls_upsample_cloud: ") + hipGetErrorString(e)); }
    }
    return rc;
  }
  hipStream_t s = ctx->stream;
  ope_cloud *c = new ope_cloud();
  c->ctx = ctx;
  c->n = m;
  c->n_valid = o.n_finite;
  c->host_valid = false;
  std::memcpy(c->bb_lo, o.lo, sizeof o.lo);
  std::memcpy(c->bb_hi, o.hi, sizeof o.hi);
  int32_t *d_perm = nullptr;
  hipError_t e = hipMalloc((void **)&c->d_xyzw, sizeof(float4) * m);
  if (e == hipSuccess && o.d_rgb_raw) e = hipMalloc((void **)&c->d_rgb, 4 * m);
  if (e == hipSuccess && params->compute_normals) e = hipMalloc((void **)&c->d_nrm, sizeof(float4) * m);
  if (e == hipSuccess) e = tmp_malloc(s, (void **)&d_perm, 4 * m);
  if (e == hipSuccess) {
    float inv[3];
    for (int d = 0; d < 3; ++d) inv[d] = (o.hi[d] > o.lo[d]) ? 1023.999f / (o.hi[d] - o.lo[d]) : 0.f;
    e = morton_order_device(s, o.d_raw, m, o.lo, inv, c->d_xyzw, d_perm, o.d_rgb_raw, o.d_rgb_raw ? c->d_rgb : nullptr);
  }
  if (e == hipSuccess && c->d_nrm) e = mls_normals_gather(s, o.d_nrm, d_perm, (uint32_t)m, c->d_nrm);
  if (e == hipSuccess && out_idx) e = hipMemcpyAsync(out_idx, o.d_idx, 4 * m, hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  if (e == hipSuccess) e = e2;
  tmp_free(s, d_perm);
  upsample_release(ctx, o);
  if (e != hipSuccess) {
    ope_cloud_free(c);
    return set_err(ctx, OPE_EHIP, std::string("ope_mls_upsample_cloud: ") + hipGetErrorString(e));
  }
  *out = c;
  *n_out = m;
  return OPE_OK;
}

extern "C" int ope_mls_upsample_last_stats(const ope_ctx *ctx, ope_mls_upsample_stats *out) {
  if (!ctx || !out) return OPE_EINVAL;
  *out = ctx->mls_upsample_stats;
  return OPE_OK;
}
