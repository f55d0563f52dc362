// feature_math.hpp — the per-point arithmetic of the coarse stage, shared by the single-cloud kernels (features.hip) and the
// batched ones (coarse_batch.hip), so that both run the same operations: PCL's eigen33 (smallest eigenpair), the covariance
// of NormalEstimation, computePairFeatures and the SPFH binning (PCL 1.7.x normal_3d.hpp, centroid.hpp, eigen.hpp, pfh.cpp,
// fpfh.hpp).
#pragma once

#include "bvh_traverse.hpp"
#include "libm_f32.hpp"

namespace ope {

// pcl::eigen33 / computeRoots (common/impl/eigen.hpp), Scalar = float
__device__ void compute_roots2(float b, float c, float roots[3]) {
  roots[0] = 0.f;
  float d = (float)(b * b - 4.0 * c);
  if (d < 0.0f) d = 0.0f;
  const float sd = sqrtf(d);
  roots[2] = 0.5f * (b + sd);
  roots[1] = 0.5f * (b - sd);
}

__device__ void compute_roots(const float m[9], float roots[3]) {
  const float c0 = m[0] * m[4] * m[8] + 2.f * m[1] * m[2] * m[5] - m[0] * m[5] * m[5] - m[4] * m[2] * m[2] - m[8] * m[1] * m[1];
  const float c1 = m[0] * m[4] - m[1] * m[1] + m[0] * m[8] - m[2] * m[2] + m[4] * m[8] - m[5] * m[5];
  const float c2 = m[0] + m[4] + m[8];
  if (fabsf(c0) < 1.1920929e-07f) {
    compute_roots2(c2, c1, roots);
    return;
  }
  const float s_inv3 = (float)(1.0 / 3.0);
  const float s_sqrt3 = sqrtf(3.0f);
  const float c2_over_3 = c2 * s_inv3;
  float a_over_3 = (c1 - c2 * c2_over_3) * s_inv3;
  if (a_over_3 > 0.f) a_over_3 = 0.f;
  const float half_b = 0.5f * (c0 + c2_over_3 * (2.f * c2_over_3 * c2_over_3 - c1));
  float q = half_b * half_b + a_over_3 * a_over_3 * a_over_3;
  if (q > 0.f) q = 0.f;
  const float rho = sqrtf(-a_over_3);
  const float theta = lmf_atan2f(sqrtf(-q), half_b) * s_inv3;   // libm_f32.hpp: the same bits as the CPU path
  float cos_theta, sin_theta;
  lmf_cos_sin_small(theta, &cos_theta, &sin_theta);
  roots[0] = c2_over_3 + 2.f * rho * cos_theta;
  roots[1] = c2_over_3 - rho * (cos_theta + s_sqrt3 * sin_theta);
  roots[2] = c2_over_3 - rho * (cos_theta - s_sqrt3 * sin_theta);
  float t;
  if (roots[0] >= roots[1]) { t = roots[0]; roots[0] = roots[1]; roots[1] = t; }
  if (roots[1] >= roots[2]) {
    t = roots[1]; roots[1] = roots[2]; roots[2] = t;
    if (roots[0] >= roots[1]) { t = roots[0]; roots[0] = roots[1]; roots[1] = t; }
  }
  if (roots[0] <= 0.f) compute_roots2(c2, c1, roots);
}

__device__ void eigen33_smallest(const float mat[9], float *eigenvalue, float evec[3]) {
  float scale = 0.f;
#pragma unroll
  for (int i = 0; i < 9; ++i) scale = fmaxf(scale, fabsf(mat[i]));
  if (scale <= 1.17549435e-38f) scale = 1.0f;
  float sm[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) sm[i] = mat[i] / scale;
  float roots[3];
  compute_roots(sm, roots);
  *eigenvalue = roots[0] * scale;
  sm[0] -= roots[0]; sm[4] -= roots[0]; sm[8] -= roots[0];
  const float v1[3] = {sm[1] * sm[5] - sm[2] * sm[4], sm[2] * sm[3] - sm[0] * sm[5], sm[0] * sm[4] - sm[1] * sm[3]};
  const float v2[3] = {sm[1] * sm[8] - sm[2] * sm[7], sm[2] * sm[6] - sm[0] * sm[8], sm[0] * sm[7] - sm[1] * sm[6]};
  const float v3[3] = {sm[4] * sm[8] - sm[5] * sm[7], sm[5] * sm[6] - sm[3] * sm[8], sm[3] * sm[7] - sm[4] * sm[6]};
  const float l1 = v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2];
  const float l2 = v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2];
  const float l3 = v3[0] * v3[0] + v3[1] * v3[1] + v3[2] * v3[2];
  float vx, vy, vz, l;
  if (l1 >= l2 && l1 >= l3) { vx = v1[0]; vy = v1[1]; vz = v1[2]; l = l1; }
  else if (l2 >= l1 && l2 >= l3) { vx = v2[0]; vy = v2[1]; vz = v2[2]; l = l2; }
  else { vx = v3[0]; vy = v3[1]; vz = v3[2]; l = l3; }
  const float s = sqrtf(l);
  evec[0] = vx / s; evec[1] = vy / s; evec[2] = vz / s;
}

// The same algorithm with Scalar = double (MovingLeastSquares calls pcl::eigen33 on a Matrix3d, mls.hip).  The fp32 path above keeps
// its own libm (bit parity with the CPU oracle); here atan2 / cos / sin are the device library's fp64 functions.
__device__ inline void compute_roots2(double b, double c, double roots[3]) {
  roots[0] = 0.0;
  double d = b * b - 4.0 * c;
  if (d < 0.0) d = 0.0;
  const double sd = sqrt(d);
  roots[2] = 0.5 * (b + sd);
  roots[1] = 0.5 * (b - sd);
}

__device__ inline void compute_roots(const double m[9], double roots[3]) {
  const double c0 = m[0] * m[4] * m[8] + 2.0 * m[1] * m[2] * m[5] - m[0] * m[5] * m[5] - m[4] * m[2] * m[2] - m[8] * m[1] * m[1];
  const double c1 = m[0] * m[4] - m[1] * m[1] + m[0] * m[8] - m[2] * m[2] + m[4] * m[8] - m[5] * m[5];
  const double c2 = m[0] + m[4] + m[8];
  if (fabs(c0) < 2.220446049250313e-16) {
    compute_roots2(c2, c1, roots);
    return;
  }
  const double s_inv3 = 1.0 / 3.0;
  const double s_sqrt3 = sqrt(3.0);
  const double c2_over_3 = c2 * s_inv3;
  double a_over_3 = (c1 - c2 * c2_over_3) * s_inv3;
  if (a_over_3 > 0.0) a_over_3 = 0.0;
  const double half_b = 0.5 * (c0 + c2_over_3 * (2.0 * c2_over_3 * c2_over_3 - c1));
  double q = half_b * half_b + a_over_3 * a_over_3 * a_over_3;
  if (q > 0.0) q = 0.0;
  const double rho = sqrt(-a_over_3);
  const double theta = atan2(sqrt(-q), half_b) * s_inv3;
  const double cos_theta = cos(theta), sin_theta = sin(theta);
  roots[0] = c2_over_3 + 2.0 * rho * cos_theta;
  roots[1] = c2_over_3 - rho * (cos_theta + s_sqrt3 * sin_theta);
  roots[2] = c2_over_3 - rho * (cos_theta - s_sqrt3 * sin_theta);
  double t;
  if (roots[0] >= roots[1]) { t = roots[0]; roots[0] = roots[1]; roots[1] = t; }
  if (roots[1] >= roots[2]) {
    t = roots[1]; roots[1] = roots[2]; roots[2] = t;
    if (roots[0] >= roots[1]) { t = roots[0]; roots[0] = roots[1]; roots[1] = t; }
  }
  if (roots[0] <= 0.0) compute_roots2(c2, c1, roots);
}

__device__ inline void eigen33_smallest(const double mat[9], double *eigenvalue, double evec[3]) {
  double scale = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) scale = fmax(scale, fabs(mat[i]));
  if (scale <= 2.2250738585072014e-308) scale = 1.0;
  double sm[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) sm[i] = mat[i] / scale;
  double roots[3];
  compute_roots(sm, roots);
  *eigenvalue = roots[0] * scale;
  sm[0] -= roots[0]; sm[4] -= roots[0]; sm[8] -= roots[0];
  const double v1[3] = {sm[1] * sm[5] - sm[2] * sm[4], sm[2] * sm[3] - sm[0] * sm[5], sm[0] * sm[4] - sm[1] * sm[3]};
  const double v2[3] = {sm[1] * sm[8] - sm[2] * sm[7], sm[2] * sm[6] - sm[0] * sm[8], sm[0] * sm[7] - sm[1] * sm[6]};
  const double v3[3] = {sm[4] * sm[8] - sm[5] * sm[7], sm[5] * sm[6] - sm[3] * sm[8], sm[3] * sm[7] - sm[4] * sm[6]};
  const double l1 = v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2];
  const double l2 = v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2];
  const double l3 = v3[0] * v3[0] + v3[1] * v3[1] + v3[2] * v3[2];
  double vx, vy, vz, l;
  if (l1 >= l2 && l1 >= l3) { vx = v1[0]; vy = v1[1]; vz = v1[2]; l = l1; }
  else if (l2 >= l1 && l2 >= l3) { vx = v2[0]; vy = v2[1]; vz = v2[2]; l = l2; }
  else { vx = v3[0]; vy = v3[1]; vz = v3[2]; l = l3; }
  const double s = sqrt(l);
  evec[0] = vx / s; evec[1] = vy / s; evec[2] = vz / s;
}

// computeMeanAndCovarianceMatrix, single pass in fp32: one neighbour P added to the nine running sums
#define OPE_ACCUMULATE_NEIGHBOUR(P)                                       \
  accu[0] += P.x * P.x; accu[1] += P.x * P.y; accu[2] += P.x * P.z;       \
  accu[3] += P.y * P.y; accu[4] += P.y * P.z; accu[5] += P.z * P.z;       \
  accu[6] += P.x; accu[7] += P.y; accu[8] += P.z

// the normal (x, y, z) and curvature (w) of query s from the sums of its count >= 3 neighbours, flipped towards the viewpoint
__device__ __forceinline__ float4 normal_from_sums(float accu[9], int count, const float4 &s, float vpx, float vpy, float vpz) {
  const float fc = (float)count;
#pragma unroll
  for (int a = 0; a < 9; ++a) accu[a] /= fc;
  float cov[9];
  cov[0] = accu[0] - accu[6] * accu[6];
  cov[1] = accu[1] - accu[6] * accu[7];
  cov[2] = accu[2] - accu[6] * accu[8];
  cov[4] = accu[3] - accu[7] * accu[7];
  cov[5] = accu[4] - accu[7] * accu[8];
  cov[8] = accu[5] - accu[8] * accu[8];
  cov[3] = cov[1]; cov[6] = cov[2]; cov[7] = cov[5];
  float ev, nv[3];
  eigen33_smallest(cov, &ev, nv);
  const float eig_sum = cov[0] + cov[4] + cov[8];
  const float curv = (eig_sum != 0.f) ? fabsf(ev / eig_sum) : 0.f;
  // flipNormalTowardsViewpoint
  const float cos_theta = (vpx - s.x) * nv[0] + (vpy - s.y) * nv[1] + (vpz - s.z) * nv[2];
  if (cos_theta < 0) { nv[0] *= -1; nv[1] *= -1; nv[2] *= -1; }
  return make_float4(nv[0], nv[1], nv[2], curv);
}

// pcl::computePairFeatures (features/src/pfh.cpp); returns false if rejected
__device__ __forceinline__ bool pair_features(float p1x, float p1y, float p1z, float n1x, float n1y, float n1z,
                                              float p2x, float p2y, float p2z, float n2x, float n2y, float n2z,
                                              float &f1, float &f2, float &f3) {
  float dx = p2x - p1x, dy = p2y - p1y, dz = p2z - p1z;
  const float f4 = sqrtf(dx * dx + dy * dy + dz * dz);
  if (f4 == 0.0f) return false;
  float ax = n1x, ay = n1y, az = n1z, bx = n2x, by = n2y, bz = n2z;
  const float angle1 = (ax * dx + ay * dy + az * dz) / f4;
  const float angle2 = (bx * dx + by * dy + bz * dz) / f4;
  if (lmf_acosf(fabsf(angle1)) > lmf_acosf(fabsf(angle2))) {   // (libm_f32.hpp: the same bits as the C library of the CPU path)
    ax = n2x; ay = n2y; az = n2z;
    bx = n1x; by = n1y; bz = n1z;
    dx *= -1.f; dy *= -1.f; dz *= -1.f;
    f3 = -angle2;
  } else {
    f3 = angle1;
  }
  float vx = dy * az - dz * ay, vy = dz * ax - dx * az, vz = dx * ay - dy * ax;
  const float vn = sqrtf(vx * vx + vy * vy + vz * vz);
  if (vn == 0.0f) return false;
  vx /= vn; vy /= vn; vz /= vn;
  const float wx = ay * vz - az * vy, wy = az * vx - ax * vz, wz = ax * vy - ay * vx;
  f2 = vx * bx + vy * by + vz * bz;
  f1 = lmf_atan2f(wx * bx + wy * by + wz * bz, ax * bx + ay * by + az * bz);
  return true;
}

// SPFH binning (computePointSPFHSignature): the bin, 0..10 within its 11-bin group, of the angle feature f1 and of the
// features f2 and f3 in [-1, 1]
__device__ __forceinline__ int spfh_bin_angle(float f1) {
  const double d_pi = (double)(1.0f / (2.0f * 3.14159274f));
  const int h = (int)floor(11 * (((double)f1 + 3.14159265358979323846) * d_pi));
  return min(max(h, 0), 10);
}
__device__ __forceinline__ int spfh_bin_unit(float f) {
  const int h = (int)floor(11 * (((double)f + 1.0) * 0.5));
  return min(max(h, 0), 10);
}

// findSimilarFeatures of one query descriptor (a 256-thread block): the k nearest of the nt target descriptors (33-D,
// squared L2, fp32 sequential sum), ties by index.  Every thread keeps its kFeatK best, thread 0 merges by (d, index).
constexpr int kFeatK = 8;
__device__ __forceinline__ void feature_knn_block(const float *__restrict__ tgt_feat, int nt, const float *__restrict__ q_row, int k,
                                                  int32_t *__restrict__ out_row) {
  __shared__ float s_d[256][kFeatK];
  __shared__ int s_i[256][kFeatK];
  __shared__ float s_q[33];
  if (threadIdx.x < 33) s_q[threadIdx.x] = q_row[threadIdx.x];
  __syncthreads();
  float bd[kFeatK];
  int bi[kFeatK];
#pragma unroll
  for (int j = 0; j < kFeatK; ++j) { bd[j] = INFINITY; bi[j] = -1; }
  for (int t = threadIdx.x; t < nt; t += 256) {
    const float *f = tgt_feat + (size_t)t * 33;
    float d = 0.f;
    for (int c = 0; c < 33; ++c) { const float u = s_q[c] - f[c]; d += u * u; }
    if (!(d == d)) continue;  // NaN descriptors never match
    if (d < bd[kFeatK - 1]) {
      bd[kFeatK - 1] = d; bi[kFeatK - 1] = t;
#pragma unroll
      for (int j = kFeatK - 1; j > 0; --j)
        if (bd[j - 1] > bd[j]) {
          const float td = bd[j]; bd[j] = bd[j - 1]; bd[j - 1] = td;
          const int ti = bi[j]; bi[j] = bi[j - 1]; bi[j - 1] = ti;
        }
    }
  }
#pragma unroll
  for (int j = 0; j < kFeatK; ++j) { s_d[threadIdx.x][j] = bd[j]; s_i[threadIdx.x][j] = bi[j]; }
  __syncthreads();
  __shared__ unsigned char cur[256];
  cur[threadIdx.x] = 0;
  __syncthreads();
  if (threadIdx.x == 0) {
    // k-way selection by (distance, index): k <= 8 passes over the 256 list heads
    for (int r = 0; r < k; ++r) {
      float best = INFINITY;
      int best_i = -1, best_t = -1;
      for (int t = 0; t < 256; ++t) {
        const int c = cur[t];
        if (c >= kFeatK) continue;
        const float d = s_d[t][c];
        const int id = s_i[t][c];
        if (id < 0) continue;
        if (d < best || (d == best && id < best_i)) { best = d; best_i = id; best_t = t; }
      }
      out_row[r] = best_i;
      if (best_t >= 0) cur[best_t]++;
    }
  }
}

}  // namespace ope
