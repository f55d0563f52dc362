// mls.hip — pcl::MovingLeastSquares::process with upsampling NONE (ProcessingPcd::getSmooth, BuildModel/src/processingpcd.cpp:80-108;
// surface/include/pcl/surface/impl/mls.hpp computeMLSPointNormal), on the device.
//
// One lane per query, two walks of the cloud's own tree, each from the query's own leaf (features.hip: self_leaves), neither
// with a neighbour list: a dense model has thousands of points within the reference's 2 cm.
//   mls_plane_kernel  walk A: count, first and second moments of (p - q) in fp64 (shifted by the query: no cancellation of raw
//                     moments) -> compute3DCentroid, computeCovarianceMatrix, pcl::eigen33 (feature_math.hpp, Scalar = double),
//                     the plane, the projected query, the curvature.
//   mls_fit_kernel    walk B: the weighted moments sum w u^a v^b (a + b <= 2 * order) and right-hand sums sum w f u^a v^b
//                     (a + b <= order) about the projected query in the plane's Darboux frame; P W P^T is made of the moments;
//                     Eigen's unblocked lower Cholesky and its two triangular solves, in the lane.
// The upsampling (mls_upsample.hip) runs the same two walks in record mode for orders 0 to 4 (mls_fit_records): nothing
// moves, every point with 3 or more neighbours gets its MLSResult under its original index.
// Results go to the point's ORIGINAL index; a flag per original index, one rocPRIM scan and one scatter put the survivors in
// ascending original index (PCL's output order) with their indices and colour words.  The sequence of launches does not depend
// on the points.  The host waits once for what it needs to go on (the count, the bounding box and the statistics) and once more at the
// end of the call: for the copies to the caller's arrays, or for the new cloud (whose Morton ordering has a wait of its own, as for
// every cloud made on the device).
#include <cstring>
#include <string>

#include <rocprim/rocprim.hpp>

#include <cmath>
#include <utility>
#include <vector>

#include "feature_math.hpp"
#include "mls_shared.hpp"

namespace ope {

constexpr int kMlsBlock = 256;

struct MlsPlaneVisitor {
  float r2;
  double qx, qy, qz;
  int count;
  double s[9];   // sum e (3), sum e e^T (xx xy xz yy yz zz), e = p - q
  __device__ __forceinline__ bool prune(float bound) const { return bound > r2; }
  __device__ __forceinline__ void point(float d, const v4f &p, uint32_t, uint32_t) {
    if (!(d <= r2)) return;
    ++count;
    const double ex = (double)p.x - qx, ey = (double)p.y - qy, ez = (double)p.z - qz;
    s[0] += ex; s[1] += ey; s[2] += ez;
    s[3] += ex * ex; s[4] += ex * ey; s[5] += ex * ez;
    s[6] += ey * ey; s[7] += ey * ez; s[8] += ez * ez;
  }
  __device__ __forceinline__ void on_node() {}
};

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(kMlsBlock) void mls_plane_kernel(CloudView q, BvhView tgt, float r2, const uint32_t *__restrict__ self_leaf,
                                                               MlsPlane *__restrict__ plane, int32_t *__restrict__ cnt,
                                                               float *__restrict__ pos_orig, float4 *__restrict__ nrm_orig,
                                                               uint32_t *__restrict__ flag_orig, uint32_t *__restrict__ stats) {
  __shared__ float s_stk[kMaxDepth + 1][kMlsBlock];
  float *stk = &s_stk[0][threadIdx.x];
  unsigned long long local_nb = 0;
  for (uint32_t i = blockIdx.x * kMlsBlock + threadIdx.x; i < q.n_valid; i += gridDim.x * kMlsBlock) {
    const float4 s = q.xyzw[i];
    const uint32_t orig = (uint32_t)__float_as_int(s.w);
    MlsPlaneVisitor v{r2, (double)s.x, (double)s.y, (double)s.z, 0, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
    bvh_traverse(tgt, s.x, s.y, s.z, v, stk, kMlsBlock, self_leaf[orig]);
    cnt[i] = v.count;
    local_nb += (unsigned long long)v.count;
    if (v.count < 3) continue;   // dropped: the flag stays 0
    // compute3DCentroid and the unnormalised computeCovarianceMatrix about it, from the moments about the query
    const double inv_n = 1.0 / (double)v.count;
    const double mx = v.s[0] * inv_n, my = v.s[1] * inv_n, mz = v.s[2] * inv_n;
    const double cx = v.qx + mx, cy = v.qy + my, cz = v.qz + mz;
    double cov[9];
    cov[0] = v.s[3] - v.s[0] * mx; cov[1] = v.s[4] - v.s[0] * my; cov[2] = v.s[5] - v.s[0] * mz;
    cov[4] = v.s[6] - v.s[1] * my; cov[5] = v.s[7] - v.s[1] * mz; cov[8] = v.s[8] - v.s[2] * mz;
    cov[3] = cov[1]; cov[6] = cov[2]; cov[7] = cov[5];
    double ev, nv[3];
    eigen33_smallest(cov, &ev, nv);
    const double d4 = -1.0 * (nv[0] * cx + nv[1] * cy + nv[2] * cz);
    const double dist = (v.qx * nv[0] + v.qy * nv[1] + v.qz * nv[2]) + d4;
    MlsPlane pl;
    pl.pt[0] = v.qx - dist * nv[0]; pl.pt[1] = v.qy - dist * nv[1]; pl.pt[2] = v.qz - dist * nv[2];
    pl.n[0] = nv[0]; pl.n[1] = nv[1]; pl.n[2] = nv[2];
    plane[i] = pl;
    // mls.hpp: curvature = float(trace); if (curvature != 0) curvature = fabsf(float(eigen_value / double(curvature)))
    float curv = (float)(cov[0] + cov[4] + cov[8]);
    if (curv != 0.f) curv = fabsf((float)(ev / (double)curv));
    pos_orig[3 * (size_t)orig] = (float)pl.pt[0]; pos_orig[3 * (size_t)orig + 1] = (float)pl.pt[1]; pos_orig[3 * (size_t)orig + 2] = (float)pl.pt[2];
    nrm_orig[orig] = make_float4((float)nv[0], (float)nv[1], (float)nv[2], curv);
    flag_orig[orig] = 1u;
  }
  local_nb = wave_sum_u64(local_nb);
  if ((threadIdx.x & 63u) == 0 && local_nb) atomicAdd(reinterpret_cast<unsigned long long *>(stats + kMlsNeighbours), local_nb);
}

// the polynomial's terms u^a v^b in PCL's order (a outer 0..order, b inner 0..order - a), and the moments' slots
__host__ __device__ constexpr int mls_nr_coeff(int order) { return (order + 1) * (order + 2) / 2; }
__host__ __device__ constexpr int mls_slot(int degree, int a, int b) { return a * (degree + 1) - a * (a - 1) / 2 + b; }
__host__ __device__ constexpr int mls_term_a(int order, int j) {
  int a = 0;
  while (j >= order - a + 1) { j -= order - a + 1; ++a; }
  return a;
}
__host__ __device__ constexpr int mls_term_b(int order, int j) {
  int a = 0;
  while (j >= order - a + 1) { j -= order - a + 1; ++a; }
  return j;
}

template <int ORDER>
struct MlsFitVisitor {
  static constexpr int D = 2 * ORDER, NM = mls_nr_coeff(2 * ORDER), NR = mls_nr_coeff(ORDER);
  float r2;
  double px, py, pz, ux, uy, uz, vx, vy, vz, nx, ny, nz, sgp;
  double mom[NM], rhs[NR];
  __device__ __forceinline__ bool prune(float bound) const { return bound > r2; }
  __device__ __forceinline__ void point(float d, const v4f &p, uint32_t, uint32_t) {
    if (!(d <= r2)) return;
    const double dx = (double)p.x - px, dy = (double)p.y - py, dz = (double)p.z - pz;
    const float sq = (float)(dx * dx + dy * dy + dz * dz);
    const double w = exp((double)(-sq) / sgp);
    const double uc = dx * ux + dy * uy + dz * uz, vc = dx * vx + dy * vy + dz * vz, f = dx * nx + dy * ny + dz * nz;
    double up = w;   // w u^a
#pragma unroll
    for (int a = 0; a <= D; ++a) {
      double t = up;   // w u^a v^b
#pragma unroll
      for (int b = 0; b <= D - a; ++b) {
        mom[mls_slot(D, a, b)] += t;
        if (a + b <= ORDER) rhs[mls_slot(ORDER, a, b)] += t * f;
        t *= vc;
      }
      up *= uc;
    }
  }
  __device__ __forceinline__ void on_node() {}
};

// Eigen::LLT of the N x N matrix whose lower triangle is in A (internal::llt_inplace<Lower>::unblocked), then solveInPlace: b <- A^-1 b.
// false: a pivot that is <= 0 or not finite (Eigen would go on; here the fit counts as failed, like a non-finite c[0]).
template <int N>
__device__ __forceinline__ bool mls_llt_solve(double (&A)[N][N], double (&b)[N]) {
  // every loop has constant bounds and a guard, so that all of them unroll at once and every index is a constant (the system then
  // lives in registers for every order, the 15 x 15 of order 4 included: DESIGN.md 4.14, 4.15); a failed pivot only poisons what
  // follows, and the result is not used
  bool ok = true;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double x = A[k][k];
    double sq = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (j < k) sq += A[k][j] * A[k][j];
    if (k > 0) x -= sq;
    ok = ok && x > 0.0 && isfinite(x);
    x = sqrt(x);
    A[k][k] = x;
    const double rx = 1.0 / x;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (i <= k) continue;
      double dot = 0.0;
#pragma unroll
      for (int j = 0; j < N; ++j)
        if (j < k) dot += A[i][j] * A[k][j];
      if (k > 0) A[i][k] -= dot;
      A[i][k] *= rx;
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {   // L y = b
    double t = b[i];
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (j < i) t -= A[i][j] * b[j];
    b[i] = t / A[i][i];
  }
#pragma unroll
  for (int r = 0; r < N; ++r) {   // L^T x = y
    const int i = N - 1 - r;
    double t = b[i];
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (j > i) t -= A[j][i] * b[j];
    b[i] = t / A[i][i];
  }
  return ok;
}

// the normal equations from the sums, every slot a compile-time constant
template <int ORDER, int I, int J>
struct MlsPair {
  static constexpr int slot = mls_slot(2 * ORDER, mls_term_a(ORDER, I) + mls_term_a(ORDER, J), mls_term_b(ORDER, I) + mls_term_b(ORDER, J));
};
// (a class member, like MlsPair::slot, is a constant expression by force; a call of the constexpr functions in the subscript is one only
// if the optimiser folds their loops, and where it did not the subscript was computed at run time, the visitor stayed in private stack
// and every accumulator was stored there again for every neighbour of the walk)
template <int ORDER, int J>
struct MlsTerm {
  static constexpr int slot = mls_slot(ORDER, mls_term_a(ORDER, J), mls_term_b(ORDER, J));
};
template <int ORDER, int N, int... K>
__device__ __forceinline__ void mls_fill_system(const double *mom, const double *rhs, double (&A)[N][N], double (&c)[N],
                                                std::integer_sequence<int, K...>) {
  ((A[K / N][K % N] = mom[MlsPair<ORDER, K / N, K % N>::slot]), ...);
  ((c[K % N] = rhs[MlsTerm<ORDER, K % N>::slot]), ...);
}

// RECORD (the upsampling, mls_upsample.hip): nothing moves; every point with 3 or more neighbours gets its MLSResult under its original
// index, and `compute_normals` carries polynomial_fit instead (without it, or below nr_coeff neighbours, the record has no axes).
template <int ORDER, bool RECORD = false>
__global__ __launch_bounds__(kMlsBlock) void mls_fit_kernel(CloudView q, BvhView tgt, float r2, double sgp, int compute_normals,
                                                             const uint32_t *__restrict__ self_leaf, const MlsPlane *__restrict__ plane,
                                                             const int32_t *__restrict__ cnt, float *__restrict__ pos_orig,
                                                             float4 *__restrict__ nrm_orig, uint32_t *__restrict__ stats,
                                                             MlsRecord *__restrict__ rec = nullptr) {
  using V = MlsFitVisitor<ORDER>;
  constexpr int NR = V::NR;
  __shared__ float s_stk[kMaxDepth + 1][kMlsBlock];
  float *stk = &s_stk[0][threadIdx.x];
  uint32_t local_fit = 0;
  for (uint32_t i = blockIdx.x * kMlsBlock + threadIdx.x; i < q.n_valid; i += gridDim.x * kMlsBlock) {
    if (cnt[i] < (RECORD || NR <= 3 ? 3 : NR)) continue;   // dropped by the plane kernel, or too few neighbours for this order: its projection stands
    const float4 s = q.xyzw[i];
    const uint32_t orig = (uint32_t)__float_as_int(s.w);
    const MlsPlane pl = plane[i];
    if constexpr (RECORD) {
      MlsRecord *r = rec + orig;
#pragma unroll
      for (int d = 0; d < 3; ++d) { r->mean[d] = pl.pt[d]; r->n[d] = pl.n[d]; }
      r->m = cnt[i];
      r->curvature = reinterpret_cast<const float *>(nrm_orig + orig)[3];
      r->flags = 0u;
      if (!compute_normals || cnt[i] < NR) continue;
    }
    const double nx = pl.n[0], ny = pl.n[1], nz = pl.n[2];
    // Eigen's unitOrthogonal (3-vectors), then u = n x v
    double vx, vy, vz;
    if (fabs(nx) > fabs(nz) * 1e-12 || fabs(ny) > fabs(nz) * 1e-12) {
      const double invnm = 1.0 / sqrt(nx * nx + ny * ny);
      vx = -ny * invnm; vy = nx * invnm; vz = 0.0;
    } else {
      const double invnm = 1.0 / sqrt(ny * ny + nz * nz);
      vx = 0.0; vy = -nz * invnm; vz = ny * invnm;
    }
    const double ux = ny * vz - nz * vy, uy = nz * vx - nx * vz, uz = nx * vy - ny * vx;
    V v;
    v.r2 = r2;
    v.px = pl.pt[0]; v.py = pl.pt[1]; v.pz = pl.pt[2];
    v.ux = ux; v.uy = uy; v.uz = uz; v.vx = vx; v.vy = vy; v.vz = vz; v.nx = nx; v.ny = ny; v.nz = nz;
    v.sgp = sgp;
#pragma unroll
    for (int k = 0; k < V::NM; ++k) v.mom[k] = 0.0;
#pragma unroll
    for (int k = 0; k < NR; ++k) v.rhs[k] = 0.0;
    bvh_traverse(tgt, s.x, s.y, s.z, v, stk, kMlsBlock, self_leaf[orig]);
    // (P W P^T)(i, j) = sum w u^(a_i + a_j) v^(b_i + b_j); P W f = the right-hand sums
    double A[NR][NR], c[NR];
    mls_fill_system<ORDER>(v.mom, v.rhs, A, c, std::make_integer_sequence<int, NR * NR>());
    const bool solved = mls_llt_solve<NR>(A, c);
    if constexpr (RECORD) {
      MlsRecord *r = rec + orig;
#pragma unroll
      for (int k = 0; k < NR; ++k) r->c[k] = c[k];
      r->flags = kMlsRecAxes | (solved ? kMlsRecSolved : 0u);
      local_fit += solved ? 1u : 0u;
      continue;
    }
    if (!solved || !isfinite(c[0])) continue;   // the plane kernel's projection stands
    ++local_fit;
    const double ox = pl.pt[0] + c[0] * nx, oy = pl.pt[1] + c[0] * ny, oz = pl.pt[2] + c[0] * nz;
    pos_orig[3 * (size_t)orig] = (float)ox; pos_orig[3 * (size_t)orig + 1] = (float)oy; pos_orig[3 * (size_t)orig + 2] = (float)oz;
    if constexpr (ORDER >= 1) {
      if (compute_normals) {   // normal = plane_normal - c[order + 1] * u_axis - c[1] * v_axis, neither normalised nor oriented
        float *o = reinterpret_cast<float *>(nrm_orig + orig);
        const double cu = c[ORDER + 1], cv = c[1];
        o[0] = (float)((nx - cu * ux) - cv * vx); o[1] = (float)((ny - cu * uy) - cv * vy); o[2] = (float)((nz - cu * uz) - cv * vz);
      }
    }
  }
  const unsigned long long fit = wave_sum_u64(local_fit);
  if ((threadIdx.x & 63u) == 0 && fit) atomicAdd(stats + kMlsFit, (uint32_t)fit);
}

// bounding box and count of the FINITE results (what the new cloud's Morton order needs), by original index
__global__ __launch_bounds__(256) void mls_bbox_kernel(const float *__restrict__ pos_orig, const uint32_t *__restrict__ flag_orig, uint32_t n,
                                                        uint32_t *__restrict__ stats) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  float v[3] = {0.f, 0.f, 0.f};
  bool fin = false;
  if (i < n && flag_orig[i]) {
    v[0] = pos_orig[3 * (size_t)i]; v[1] = pos_orig[3 * (size_t)i + 1]; v[2] = pos_orig[3 * (size_t)i + 2];
    fin = isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]);
  }
  const unsigned long long m = __ballot(fin);
  if (m == 0ull) return;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const uint32_t u = (uint32_t)__float_as_int(v[d]);
    const uint32_t key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // order-preserving integer key
    uint32_t lo = fin ? key : 0xffffffffu, hi = fin ? key : 0u;
    for (int off = 32; off >= 1; off >>= 1) {
      lo = min(lo, (uint32_t)__shfl_xor((int)lo, off, 64));
      hi = max(hi, (uint32_t)__shfl_xor((int)hi, off, 64));
    }
    if ((threadIdx.x & 63u) == 0) { atomicMin(stats + kMlsMin + d, lo); atomicMax(stats + kMlsMax + d, hi); }
  }
  if ((threadIdx.x & 63u) == 0) atomicAdd(stats + kMlsFinite, (uint32_t)__popcll(m));
}

// the survivors in ascending original index: point, normal + curvature, index, and the colour word in the same launch
__global__ __launch_bounds__(256) void mls_scatter_kernel(CloudView c, const uint32_t *__restrict__ flag_orig, const uint32_t *__restrict__ rank,
                                                           const float *__restrict__ pos_orig, const float4 *__restrict__ nrm_orig,
                                                           const uint32_t *__restrict__ rgb_in, float *__restrict__ raw, float4 *__restrict__ nrm_out,
                                                           int32_t *__restrict__ idx_out, uint32_t *__restrict__ rgb_raw) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= c.n_valid) return;
  const uint32_t o = (uint32_t)__float_as_int(c.xyzw[p].w);
  if (!flag_orig[o]) return;
  const uint32_t dst = rank[o];
  raw[3 * (size_t)dst] = pos_orig[3 * (size_t)o]; raw[3 * (size_t)dst + 1] = pos_orig[3 * (size_t)o + 1]; raw[3 * (size_t)dst + 2] = pos_orig[3 * (size_t)o + 2];
  nrm_out[dst] = nrm_orig[o];
  idx_out[dst] = (int32_t)o;
  if (rgb_raw) rgb_raw[dst] = rgb_in[p];
}

// the new cloud's normals in ITS sorted order
__global__ __launch_bounds__(256) void mls_normals_gather_kernel(const float4 *__restrict__ nrm_out, const int32_t *__restrict__ perm, uint32_t n,
                                                                  float4 *__restrict__ nrm_sorted) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p < n) nrm_sorted[p] = nrm_out[perm[p]];
}

hipError_t mls_bbox(hipStream_t s, const float *d_pos, const uint32_t *d_flag, uint32_t n, uint32_t *d_stats) {
  hipLaunchKernelGGL(mls_bbox_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, d_pos, d_flag, n, d_stats);
  return hipGetLastError();
}

hipError_t mls_normals_gather(hipStream_t s, const float4 *d_nrm_out, const int32_t *d_perm, uint32_t n, float4 *d_nrm_sorted) {
  hipLaunchKernelGGL(mls_normals_gather_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, d_nrm_out, d_perm, n, d_nrm_sorted);
  return hipGetLastError();
}

template <int ORDER>
static void mls_launch_records(hipStream_t s, unsigned nblocks, const ope_cloud *cloud, const ope_index *ix, float r2, double sgp, int polynomial_fit,
                               const uint32_t *d_self, const MlsPlane *d_plane, const int32_t *d_cnt, float4 *d_nrm, uint32_t *d_stats,
                               MlsRecord *d_rec) {
  hipLaunchKernelGGL((mls_fit_kernel<ORDER, true>), dim3(nblocks), dim3(kMlsBlock), 0, s, cloud->view(), ix->view(), r2, sgp, polynomial_fit, d_self,
                     d_plane, d_cnt, (float *)nullptr, d_nrm, d_stats, d_rec);
}

hipError_t mls_fit_records(ope_ctx *ctx, const ope_cloud *cloud, const ope_index *ix, const uint32_t *d_self, float r2, double sgp,
                           int polynomial_fit, int order, uint32_t *d_flag, MlsRecord *d_rec, uint32_t *d_stats) {
  const size_t n = cloud->n, nv = cloud->n_valid;
  hipStream_t s = ctx->stream;
  MlsPlane *d_plane = nullptr;
  int32_t *d_cnt = nullptr;
  float *d_pos = nullptr;
  float4 *d_nrm = nullptr;
  hipError_t e = tmp_malloc(s, (void **)&d_plane, sizeof(MlsPlane) * nv);
  if (e == hipSuccess) e = tmp_malloc(s, (void **)&d_cnt, 4 * nv);
  if (e == hipSuccess) e = tmp_malloc(s, (void **)&d_pos, 12 * n);
  if (e == hipSuccess) e = tmp_malloc(s, (void **)&d_nrm, 16 * n);
  if (e == hipSuccess) {
    const unsigned nblocks = (unsigned)std::min<size_t>((nv + kMlsBlock - 1) / kMlsBlock, 8192);
    KernelTimer kt_a(ctx, "mls_plane_kernel", 0.0), kt_b(ctx, "mls_fit_kernel", 0.0, /*start_now=*/false);
    hipLaunchKernelGGL(mls_plane_kernel, dim3(nblocks), dim3(kMlsBlock), 0, s, cloud->view(), ix->view(), r2, d_self, d_plane, d_cnt, d_pos, d_nrm,
                       d_flag, d_stats);
    kt_a.stop();
    e = hipGetLastError();
    if (e == hipSuccess) {
      kt_b.start();
      switch (order) {
        case 0: mls_launch_records<0>(s, nblocks, cloud, ix, r2, sgp, polynomial_fit, d_self, d_plane, d_cnt, d_nrm, d_stats, d_rec); break;
        case 1: mls_launch_records<1>(s, nblocks, cloud, ix, r2, sgp, polynomial_fit, d_self, d_plane, d_cnt, d_nrm, d_stats, d_rec); break;
        case 2: mls_launch_records<2>(s, nblocks, cloud, ix, r2, sgp, polynomial_fit, d_self, d_plane, d_cnt, d_nrm, d_stats, d_rec); break;
        case 3: mls_launch_records<3>(s, nblocks, cloud, ix, r2, sgp, polynomial_fit, d_self, d_plane, d_cnt, d_nrm, d_stats, d_rec); break;
        default: mls_launch_records<4>(s, nblocks, cloud, ix, r2, sgp, polynomial_fit, d_self, d_plane, d_cnt, d_nrm, d_stats, d_rec); break;
      }
      kt_b.stop();
      e = hipGetLastError();
    }
  }
  for (void *q : {(void *)d_plane, (void *)d_cnt, (void *)d_pos, (void *)d_nrm}) tmp_free(s, q);
  return e;
}

// what a call leaves on the device (temporaries of the context's stream; mls_release gives them back)
struct MlsOut {
  float *d_raw = nullptr;        // count * 3, ascending original index
  float4 *d_nrm = nullptr;       // count: normal, curvature
  int32_t *d_idx = nullptr;      // count
  uint32_t *d_rgb_raw = nullptr; // count, when the input has colours
  size_t count = 0;
  uint32_t n_finite = 0;
  float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
};

static void mls_release(ope_ctx *ctx, MlsOut &o) {
  for (void *p : {(void *)o.d_raw, (void *)o.d_nrm, (void *)o.d_idx, (void *)o.d_rgb_raw}) tmp_free(ctx->stream, p);
  o = MlsOut();
}

static int mls_check(ope_ctx *ctx, const ope_cloud *cloud, const ope_mls_params *p, const char *who) {
  if (!ctx || !cloud || !p) return set_err(ctx, OPE_EINVAL, std::string(who) + ": bad argument");
  if (!(p->radius > 0) || !std::isfinite(p->radius) || !((float)p->radius * (float)p->radius > 0.f))
    return set_err(ctx, OPE_EINVAL, std::string(who) + ": the radius must be positive");
  if (p->order < 0 || p->order > 2) return set_err(ctx, OPE_EINVAL, std::string(who) + ": polynomial orders 0, 1 and 2 are supported");
  if (!(p->sqr_gauss_param >= 0) || !std::isfinite(p->sqr_gauss_param))
    return set_err(ctx, OPE_EINVAL, std::string(who) + ": sqr_gauss_param must be positive, or 0 for radius^2");
  if (cloud->n > (size_t)0x7fffffff) return set_err(ctx, OPE_EINVAL, std::string(who) + ": more than 2^31-1 points");
  return OPE_OK;
}

static int mls_core(ope_ctx *ctx, const ope_cloud *cloud, const ope_mls_params &p, MlsOut &o, const char *who) {
  const size_t n = cloud->n, nv = cloud->n_valid;
  ope_mls_stats &st = ctx->mls_stats;
  st = ope_mls_stats{(int64_t)n, 0, 0, (int64_t)n, 0};
  if (nv == 0) return OPE_OK;
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  TraceRange r(ctx, "mls");
  ope_index *ix = nullptr;
  ope_index_params ip;
  ope_index_default_params(&ip);
  ip.grid = 0;   // the index serves the two walks of this call
  int rc = index_build_tmp(ctx, cloud, &ip, &ix);
  if (rc != OPE_OK) return rc;
  uint32_t *d_self = nullptr, *d_flag = nullptr, *d_rank = nullptr, *d_stats = nullptr;
  MlsPlane *d_plane = nullptr;
  int32_t *d_cnt = nullptr;
  float *d_pos = nullptr;
  float4 *d_nrm = nullptr;
  void *d_tmp = nullptr;
  size_t tb = 0;
  uint32_t init[kMlsWords] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, res[kMlsWords];
  uint32_t count = 0;
  hipError_t e = tmp_malloc(s, (void **)&d_self, 4 * n);
  if (e == hipSuccess) e = tmp_malloc(s, (void **)&d_flag, 4 * (n + 1));
  if (e == hipSuccess) e = tmp_malloc(s, (void **)&d_rank, 4 * (n + 1));
  if (e == hipSuccess) e = tmp_malloc(s, (void **)&d_stats, sizeof init);
  if (e == hipSuccess) e = tmp_malloc(s, (void **)&d_plane, sizeof(MlsPlane) * nv);
  if (e == hipSuccess) e = tmp_malloc(s, (void **)&d_cnt, 4 * nv);
  if (e == hipSuccess) e = tmp_malloc(s, (void **)&d_pos, 12 * n);
  if (e == hipSuccess) e = tmp_malloc(s, (void **)&d_nrm, 16 * n);
  if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, tb, d_flag, d_rank, 0u, n + 1, rocprim::plus<uint32_t>(), s);
  if (e == hipSuccess) e = tmp_malloc(s, &d_tmp, std::max<size_t>(tb, 16));
  if (e == hipSuccess) e = self_leaves(s, ix->view(), n, d_self);
  if (e == hipSuccess) e = hipMemsetAsync(d_flag, 0, 4 * (n + 1), s);
  if (e == hipSuccess) e = h2d_copy(s, d_stats, init, sizeof init);
  if (e == hipSuccess) {
    const float r2 = (float)p.radius * (float)p.radius;
    const double sgp = p.sqr_gauss_param != 0.0 ? p.sqr_gauss_param : p.radius * p.radius;   // setSearchRadius: sqr_gauss_param_ = radius^2
    const unsigned nblocks = (unsigned)std::min<size_t>((nv + kMlsBlock - 1) / kMlsBlock, 8192);
    // algorithmic bytes (set once the neighbour count is known): a walk reads 16 bytes per neighbour; walk A also reads the query and
    // its leaf (20) and writes the plane, the count, the result and the flag (48 + 4 + 12 + 16 + 4); walk B reads the query, its
    // leaf, the count and the plane (72) and writes the result (12, 24 with normals)
    KernelTimer kt_a(ctx, "mls_plane_kernel", 0.0, /*start_now=*/false), kt_b(ctx, "mls_fit_kernel", 0.0, /*start_now=*/false);
    kt_a.start();
    hipLaunchKernelGGL(mls_plane_kernel, dim3(nblocks), dim3(kMlsBlock), 0, s, cloud->view(), ix->view(), r2, d_self, d_plane, d_cnt, d_pos, d_nrm,
                       d_flag, d_stats);
    kt_a.stop();
    e = hipGetLastError();
    if (e == hipSuccess && p.polynomial_fit) {
      kt_b.start();
      if (p.order == 0)
        hipLaunchKernelGGL(mls_fit_kernel<0>, dim3(nblocks), dim3(kMlsBlock), 0, s, cloud->view(), ix->view(), r2, sgp, p.compute_normals, d_self,
                           d_plane, d_cnt, d_pos, d_nrm, d_stats);
      else if (p.order == 1)
        hipLaunchKernelGGL(mls_fit_kernel<1>, dim3(nblocks), dim3(kMlsBlock), 0, s, cloud->view(), ix->view(), r2, sgp, p.compute_normals, d_self,
                           d_plane, d_cnt, d_pos, d_nrm, d_stats);
      else
        hipLaunchKernelGGL(mls_fit_kernel<2>, dim3(nblocks), dim3(kMlsBlock), 0, s, cloud->view(), ix->view(), r2, sgp, p.compute_normals, d_self,
                           d_plane, d_cnt, d_pos, d_nrm, d_stats);
      kt_b.stop();
      e = hipGetLastError();
    }
    if (e == hipSuccess) {
      hipLaunchKernelGGL(mls_bbox_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_pos, d_flag, (uint32_t)n, d_stats);
      e = hipGetLastError();
    }
    size_t t1 = std::max<size_t>(tb, 16);
    if (e == hipSuccess) e = rocprim::exclusive_scan(d_tmp, t1, d_flag, d_rank, 0u, n + 1, rocprim::plus<uint32_t>(), s);
    if (e == hipSuccess) e = hipMemcpyAsync(&count, d_rank + n, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(res, d_stats, sizeof res, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // the wait for what the host needs: count, bounding box, statistics
    if (e == hipSuccess) {
      unsigned long long nb_total;
      std::memcpy(&nb_total, res + kMlsNeighbours, 8);
      kt_a.set_bytes(16.0 * (double)nb_total + 104.0 * (double)nv);
      kt_b.set_bytes(16.0 * (double)nb_total + (p.compute_normals ? 96.0 : 84.0) * (double)nv);
    }
  }
  if (e == hipSuccess && count) {
    e = tmp_malloc(s, (void **)&o.d_raw, 12 * (size_t)count);
    if (e == hipSuccess) e = tmp_malloc(s, (void **)&o.d_nrm, 16 * (size_t)count);
    if (e == hipSuccess) e = tmp_malloc(s, (void **)&o.d_idx, 4 * (size_t)count);
    if (e == hipSuccess && cloud->d_rgb) e = tmp_malloc(s, (void **)&o.d_rgb_raw, 4 * (size_t)count);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(mls_scatter_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, s, cloud->view(), d_flag, d_rank, d_pos, d_nrm,
                         (const uint32_t *)cloud->d_rgb, o.d_raw, o.d_nrm, o.d_idx, o.d_rgb_raw);
      e = hipGetLastError();
    }
  }
  for (void *q : {(void *)d_self, (void *)d_flag, (void *)d_rank, (void *)d_stats, (void *)d_plane, (void *)d_cnt, (void *)d_pos, (void *)d_nrm, d_tmp})
    tmp_free(s, q);
  ope_index_free(ix);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(s);   // (no copy into this frame may outlive it)
    mls_release(ctx, o);
    return set_err(ctx, OPE_EHIP, std::string(who) + ": " + hipGetErrorString(e));
  }
  auto unkey = [](uint32_t k) { const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; float f; std::memcpy(&f, &u, 4); return f; };
  o.count = count;
  o.n_finite = res[kMlsFinite];
  if (o.n_finite > 0)
    for (int d = 0; d < 3; ++d) { o.lo[d] = unkey(res[kMlsMin + d]); o.hi[d] = unkey(res[kMlsMax + d]); }
  unsigned long long nb;
  std::memcpy(&nb, res + kMlsNeighbours, 8);
  st.n_out = (int64_t)count;
  st.n_dropped = (int64_t)n - (int64_t)count;
  st.n_plane_only = (int64_t)count - (int64_t)res[kMlsFit];
  st.neighbours_total = (int64_t)nb;
  return OPE_OK;
}

}  // namespace ope

using namespace ope;

extern "C" void ope_mls_default_params(ope_mls_params *p) {
  if (!p) return;
  p->radius = 0.0;            // MovingLeastSquares: search_radius_ (0); getSmooth passes its own (regmeshpcd.cpp:266: 0.02)
  p->polynomial_fit = 1;      // processingpcd.cpp: setPolynomialFit (true)
  p->order = 2;               // MovingLeastSquares: order_ (2)
  p->sqr_gauss_param = 0.0;   // 0: radius^2, as setSearchRadius sets it
  p->compute_normals = 0;     // MovingLeastSquares: compute_normals_ (false)
}

extern "C" int ope_mls_smooth(ope_ctx *ctx, const ope_cloud *cloud, const ope_mls_params *params, float *out_xyz, float *out_normals,
                              float *out_curvature, int32_t *out_idx, size_t *n_out) {
  if (n_out) *n_out = 0;
  if (!n_out) return set_err(ctx, OPE_EINVAL, "ope_mls_smooth: bad argument");
  int rc = mls_check(ctx, cloud, params, "ope_mls_smooth");
  if (rc != OPE_OK) return rc;
  MlsOut o;
  rc = mls_core(ctx, cloud, *params, o, "ope_mls_smooth");
  if (rc != OPE_OK) return rc;
  hipError_t e = hipSuccess;
  const size_t m = o.count;
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
  mls_release(ctx, o);
  if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string("ope_mls_smooth: ") + hipGetErrorString(e));
  *n_out = m;
  return OPE_OK;
}

extern "C" int ope_mls_smooth_cloud(ope_ctx *ctx, const ope_cloud *cloud, const ope_mls_params *params, ope_cloud **out, int32_t *out_idx,
                                    size_t *n_out) {
  if (out) *out = nullptr;
  if (n_out) *n_out = 0;
  if (!out || !n_out) return set_err(ctx, OPE_EINVAL, "ope_mls_smooth_cloud: bad argument");
  int rc = mls_check(ctx, cloud, params, "ope_mls_smooth_cloud");
  if (rc != OPE_OK) return rc;
  MlsOut o;
  rc = mls_core(ctx, cloud, *params, o, "ope_mls_smooth_cloud");
  if (rc != OPE_OK) return rc;
  const size_t m = o.count;
  if (m == 0) {
    // an empty cloud, coloured if the input was (and with the normals' buffer when they were asked for)
    OPE_HIP(ctx, hipSetDevice(ctx->device));
    rc = select_cloud_device(ctx, cloud, nullptr, 0, out);
    if (rc == OPE_OK && params->compute_normals && !(*out)->d_nrm) {
      const hipError_t e = hipMalloc((void **)&(*out)->d_nrm, sizeof(float4));
      if (e != hipSuccess) { ope_cloud_free(*out); *out = nullptr; return set_err(ctx, OPE_EHIP, std::string("ope_mls_smooth_cloud: ") + hipGetErrorString(e)); }
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
  if (e == hipSuccess && c->d_nrm)
    hipLaunchKernelGGL(mls_normals_gather_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, o.d_nrm, d_perm, (uint32_t)m, c->d_nrm);
  if (e == hipSuccess && out_idx) e = hipMemcpyAsync(out_idx, o.d_idx, 4 * m, hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  if (e == hipSuccess) e = e2;
  tmp_free(s, d_perm);
  mls_release(ctx, o);
  if (e != hipSuccess) {
    ope_cloud_free(c);
    return set_err(ctx, OPE_EHIP, std::string("ope_mls_smooth_cloud: ") + hipGetErrorString(e));
  }
  *out = c;
  *n_out = m;
  return OPE_OK;
}

extern "C" int ope_mls_last_stats(const ope_ctx *ctx, ope_mls_stats *out) {
  if (!ctx || !out) return OPE_EINVAL;
  *out = ctx->mls_stats;
  return OPE_OK;
}
