// icp_update.hpp — the ICP update step of one lane (gfx950): Umeyama / point-to-plane Cholesky from the reduced sums,
// final_T = T * final_T and PCL's convergence rule.  Shared by the per-iteration update kernels (icp_kernels.hip) and the
// batched ICP kernel (icp_batch.hip), so both paths run the very same code.
#pragma once

#include "bvh_traverse.hpp"

namespace ope {

// ------------------------------------------------------------------------------------------
// fp64 3x3 helpers for the update step (one lane)
// The update is a serial tail of every iteration, so its fp64 divisions / square roots use the
// hardware seed (v_rcp_f64 / v_rsq_f64) plus Newton steps instead of the ~40-instruction IEEE
// sequences: ~1e-16 relative error, 22 us -> a few us per iteration.
__device__ __forceinline__ double fast_rcp(double x) {
  double y = __builtin_amdgcn_rcp(x);
  y = y * (2.0 - x * y);
  y = y * (2.0 - x * y);
  return y;
}
__device__ __forceinline__ double fast_rsqrt(double x) {
  double y = __builtin_amdgcn_rsq(x);
  y = y * (1.5 - 0.5 * x * y * y);
  y = y * (1.5 - 0.5 * x * y * y);
  return y;
}
__device__ __forceinline__ double fast_sqrt(double x) { return x > 0.0 ? x * fast_rsqrt(x) : 0.0; }
// All indices below are compile-time constants after unrolling, so the 3x3 work stays in registers
// (a first version with run-time indices put 368 bytes per lane in scratch and took ~18 us).
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&S)[9], double (&V)[9]) {
  const double apq = S[3 * P + Q];
  if (apq == 0.0) return;
  const double theta = (S[3 * Q + Q] - S[3 * P + P]) * fast_rcp(2.0 * apq);
  const double t = (theta >= 0 ? 1.0 : -1.0) * fast_rcp(fabs(theta) + fast_sqrt(theta * theta + 1.0));
  const double c = fast_rsqrt(t * t + 1.0), s = t * c;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double a = S[3 * k + P], b = S[3 * k + Q];
    S[3 * k + P] = c * a - s * b;
    S[3 * k + Q] = s * a + c * b;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double a = S[3 * P + k], b = S[3 * Q + k];
    S[3 * P + k] = c * a - s * b;
    S[3 * Q + k] = s * a + c * b;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double a = V[3 * k + P], b = V[3 * k + Q];
    V[3 * k + P] = c * a - s * b;
    V[3 * k + Q] = s * a + c * b;
  }
}

// `warm`: V holds an orthonormal basis that nearly diagonalises S already (the eigenvectors of the previous ICP
// iteration's matrix): S is moved into that basis first and one or two sweeps finish the job instead of five or six
// (the update lane is a serial tail of every iteration; its fp64 instructions issue one per 8 cycles).
__device__ __forceinline__ void jacobi_eig3(double (&S)[9], double (&V)[9], bool warm = false) {
  if (warm) {
    double SV[9], W[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) SV[3 * r + c] = S[3 * r] * V[c] + S[3 * r + 1] * V[3 + c] + S[3 * r + 2] * V[6 + c];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = r; c < 3; ++c) W[3 * r + c] = V[r] * SV[c] + V[3 + r] * SV[3 + c] + V[6 + r] * SV[6 + c];
    W[3] = W[1]; W[6] = W[2]; W[7] = W[5];
#pragma unroll
    for (int i = 0; i < 9; ++i) S[i] = W[i];
  } else {
#pragma unroll
    for (int i = 0; i < 9; ++i) V[i] = (i % 4 == 0) ? 1.0 : 0.0;
  }
  for (int sweep = 0; sweep < 30; ++sweep) {
    const double off = fabs(S[1]) + fabs(S[2]) + fabs(S[5]);
    const double diag = fabs(S[0]) + fabs(S[4]) + fabs(S[8]);
    // fp64 rounding keeps `off` near 1e-17*diag forever: stop at 1e-15 (rotation error ~1e-15)
    if (off <= 1e-300 || off <= 1e-15 * diag) break;
    jacobi_rotate<0, 1>(S, V);
    jacobi_rotate<0, 2>(S, V);
    jacobi_rotate<1, 2>(S, V);
  }
}

__device__ __forceinline__ double det3(const double (&M)[9]) {
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

template <int A, int B>
__device__ __forceinline__ void sort_cols_desc(double (&ev)[3], double (&V)[9]) {
  if (ev[B] > ev[A]) {
    const double t = ev[A]; ev[A] = ev[B]; ev[B] = t;
#pragma unroll
    for (int r = 0; r < 3; ++r) { const double u = V[3 * r + A]; V[3 * r + A] = V[3 * r + B]; V[3 * r + B] = u; }
  }
}

// A = U diag(s) V^T, s descending (row-major 3x3)
// warm: V comes in holding the previous call's V (see jacobi_eig3)
__device__ __forceinline__ void svd3(const double (&A)[9], double (&U)[9], double (&s)[3], double (&V)[9], bool warm = false) {
  double AtA[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) AtA[3 * i + j] = A[i] * A[j] + A[3 + i] * A[3 + j] + A[6 + i] * A[6 + j];
  jacobi_eig3(AtA, V, warm);
  double ev[3] = {AtA[0], AtA[4], AtA[8]};
  sort_cols_desc<0, 1>(ev, V);
  sort_cols_desc<0, 2>(ev, V);
  sort_cols_desc<1, 2>(ev, V);
  // U columns = A v_c, then modified Gram-Schmidt with completion for (near-)null directions
  double u0[3], u1[3], u2[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    u0[r] = A[3 * r] * V[0] + A[3 * r + 1] * V[3] + A[3 * r + 2] * V[6];
    u1[r] = A[3 * r] * V[1] + A[3 * r + 1] * V[4] + A[3 * r + 2] * V[7];
    u2[r] = A[3 * r] * V[2] + A[3 * r + 1] * V[5] + A[3 * r + 2] * V[8];
  }
  s[0] = fast_sqrt(u0[0] * u0[0] + u0[1] * u0[1] + u0[2] * u0[2]);
  s[1] = fast_sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
  s[2] = fast_sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
  const double tiny = 1e-14 * (s[0] > 0 ? s[0] : 1.0);
  // column 0
  if (s[0] <= tiny) { u0[0] = 1; u0[1] = 0; u0[2] = 0; }
  else { const double i0 = fast_rcp(s[0]); u0[0] *= i0; u0[1] *= i0; u0[2] *= i0; }
  // column 1
  {
    const double d = u1[0] * u0[0] + u1[1] * u0[1] + u1[2] * u0[2];
    u1[0] -= d * u0[0]; u1[1] -= d * u0[1]; u1[2] -= d * u0[2];
    double n1 = fast_sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
    if (s[1] <= tiny || n1 <= 1e-8 * s[1] + 1e-300) {
      // unit vector along the axis u0 is least aligned with, made orthogonal to u0
      const double ax = fabs(u0[0]), ay = fabs(u0[1]), az = fabs(u0[2]);
      const bool mx = ax < ay ? (ax < az) : false;
      const bool my = !mx && (ax < ay ? false : (ay < az));
      const double ex = mx ? 1.0 : 0.0, ey = my ? 1.0 : 0.0, ez = (!mx && !my) ? 1.0 : 0.0;
      const double dd = ex * u0[0] + ey * u0[1] + ez * u0[2];
      u1[0] = ex - dd * u0[0]; u1[1] = ey - dd * u0[1]; u1[2] = ez - dd * u0[2];
      n1 = fast_sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
    }
    const double i1 = fast_rcp(n1);
    u1[0] *= i1; u1[1] *= i1; u1[2] *= i1;
  }
  // column 2
  {
    const double d0 = u2[0] * u0[0] + u2[1] * u0[1] + u2[2] * u0[2];
    u2[0] -= d0 * u0[0]; u2[1] -= d0 * u0[1]; u2[2] -= d0 * u0[2];
    const double d1 = u2[0] * u1[0] + u2[1] * u1[1] + u2[2] * u1[2];
    u2[0] -= d1 * u1[0]; u2[1] -= d1 * u1[1]; u2[2] -= d1 * u1[2];
    double n2 = fast_sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
    if (s[2] <= tiny || n2 <= 1e-8 * s[2] + 1e-300) {
      u2[0] = u0[1] * u1[2] - u0[2] * u1[1];
      u2[1] = u0[2] * u1[0] - u0[0] * u1[2];
      u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
      n2 = fast_sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
    }
    const double i2 = fast_rcp(n2);
    u2[0] *= i2; u2[1] *= i2; u2[2] *= i2;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) { U[3 * r] = u0[r]; U[3 * r + 1] = u1[r]; U[3 * r + 2] = u2[r]; }
}

// Eigen::umeyama(src, dst, false) from the 17 sums (taken about `pivot`), column-major fp64 out.
// Vwarm (optional): 9 doubles + a validity flag carried from one ICP iteration to the next
__device__ __forceinline__ void umeyama_from_sums(const double *S, const double *pivot, double (&T)[16], double *Vwarm = nullptr,
                                                  int *have_warm = nullptr) {
  const double n = S[0];
  double sm[3], dm[3], sigma[9];
  const double inv_n = 1.0 / n;
#pragma unroll
  for (int d = 0; d < 3; ++d) { sm[d] = S[1 + d] * inv_n; dm[d] = S[4 + d] * inv_n; }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) sigma[3 * r + c] = S[7 + 3 * r + c] * inv_n - dm[r] * sm[c];
#pragma unroll
  for (int d = 0; d < 3; ++d) { sm[d] += pivot[d]; dm[d] += pivot[d]; }
  double U[9], sv[3], V[9];
  const bool warm = Vwarm != nullptr && *have_warm != 0;
  if (warm) {
#pragma unroll
    for (int i = 0; i < 9; ++i) V[i] = Vwarm[i];
  }
  svd3(sigma, U, sv, V, warm);
  if (Vwarm != nullptr) {
#pragma unroll
    for (int i = 0; i < 9; ++i) Vwarm[i] = V[i];
    *have_warm = 1;
  }
  double Sg[3] = {1, 1, 1};
  if (det3(sigma) < 0) Sg[2] = -1;
  int rank = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (!(fabs(sv[i]) <= fabs(sv[0]) * 1e-5)) ++rank;
  if (rank == 2) {
    Sg[0] = Sg[1] = 1;
    Sg[2] = (det3(U) * det3(V) > 0) ? 1 : -1;
  } else if (rank < 2) {
    // collinear or coincident pairs: the sign of det(sigma) is rounding noise and the completed U, V come out of either
    // handedness, so U Sg V^T above could be a reflection.  R must be a rotation: the sign follows the bases themselves
    // (the rule Eigen 3.4's umeyama applies at every rank).  Ranks 2 and 3 are untouched.
    Sg[2] = (det3(U) * det3(V) < 0) ? -1 : 1;
  }
  double R[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double a = 0;
#pragma unroll
      for (int k = 0; k < 3; ++k) a += U[3 * i + k] * Sg[k] * V[3 * j + k];
      R[3 * i + j] = a;
    }
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) T[4 * c + r] = R[3 * r + c];
  T[3] = T[7] = T[11] = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) T[12 + i] = dm[i] - (R[3 * i] * sm[0] + R[3 * i + 1] * sm[1] + R[3 * i + 2] * sm[2]);
  T[15] = 1.0;
}

// x = (AᵀA)^-1 Aᵀb by Cholesky (static indices: registers only), then PCL's constructTransformationMatrix.
// N holds the upper triangle of AᵀA row by row (21 values) followed by Aᵀb (6).
__device__ __forceinline__ bool point_to_plane_from_sums(const double *N, double (&T)[16]) {
  double A[6][6], b[6];
  {
    int k = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) { A[r][c] = N[k]; A[c][r] = N[k]; ++k; }
#pragma unroll
    for (int r = 0; r < 6; ++r) b[r] = N[21 + r];
  }
  double L[6][6];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    ok = ok && (d > 0.0);
    const double inv = ok ? fast_rsqrt(d) : 0.0;
    L[j][j] = d * inv;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      L[i][j] = v * inv;
    }
  }
  if (!ok) return false;
  double yv[6], x[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double v = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= L[i][k] * yv[k];
    yv[i] = v * fast_rcp(L[i][i]);
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double v = yv[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) v -= L[k][i] * x[k];
    x[i] = v * fast_rcp(L[i][i]);
  }
  const double sa = sin(x[0]), ca = cos(x[0]), sb = sin(x[1]), cb = cos(x[1]), sg = sin(x[2]), cg = cos(x[2]);
  // column-major
  T[0] = cg * cb;                 T[4] = -sg * ca + cg * sb * sa;  T[8] = sg * sa + cg * sb * ca;   T[12] = x[3];
  T[1] = sg * cb;                 T[5] = cg * ca + sg * sb * sa;   T[9] = -cg * sa + sg * sb * ca;  T[13] = x[4];
  T[2] = -sb;                     T[6] = cb * sa;                  T[10] = cb * ca;                 T[14] = x[5];
  T[3] = 0.0; T[7] = 0.0; T[11] = 0.0; T[15] = 1.0;
  return true;
}

// Tk_ext: the incremental transform of an estimator that runs outside this kernel (LM, lm.hip), column-major float, or null
__device__ __forceinline__ void icp_update_lane(IcpState *st, const double *S, const float *Tk_ext = nullptr) {
  const double n = S[0];
  st->n_corr = (long long)n;
  // icp_mod.hpp:232-240
  if ((long long)n < (long long)st->min_correspondences) {
    st->state = OPE_CONV_NO_CORRESPONDENCES;
    st->converged = 0;
    st->done = 1;
    return;
  }
  double Tk[16];
  if (Tk_ext != nullptr) {
#pragma unroll
    for (int i = 0; i < 16; ++i) Tk[i] = (double)Tk_ext[i];
  } else if (st->estimator == OPE_EST_POINT_TO_PLANE_LLS) {
    if (!point_to_plane_from_sums(S + kNumSums, Tk)) {
      // singular normal equations: no usable step (PCL would propagate NaNs); stop with what we have
      st->state = OPE_CONV_NO_CORRESPONDENCES;
      st->converged = 0;
      st->done = 1;
      return;
    }
  } else {
    umeyama_from_sums(S, st->pivot, Tk, st->Vwarm, &st->have_Vwarm);
  }
  // transformation_ is a Matrix4f in the reference
  float Tf[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) { Tf[i] = (float)Tk[i]; st->Tk[i] = (double)Tf[i]; }
  // k-NN runs: the transform the accumulate launch behind these sums searched with (see icp_accumulate_kernel, MODE 2)
#pragma unroll
  for (int i = 0; i < 12; ++i) st->Fprev[i] = st->Ff[i];
  st->have_prev = st->knn_acc_flag;
  st->knn_acc_flag = 0;
  // final_transformation_ = transformation_ * final_transformation_ (icp_mod.hpp:249), kept in fp64
  double Fn[16];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double a = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) a += (double)Tf[4 * k + r] * st->F[4 * c + k];
      Fn[4 * c + r] = a;
    }
  {
    // Skip certificates (ope.h: skip_certificates): from the update on that moves no scene point by more than cert_thr the
    // accumulate launches keep per-query certificates.  The largest displacement over the scene's bounding sphere, centre c and
    // radius r in the scene's own frame: |Fn c - F c| + ||Rn - R||_F r (a trigger only: exactness never rests on it).  Sticky.
    const double cx = (double)st->src_c[0], cy = (double)st->src_c[1], cz = (double)st->src_c[2];
    double mv2 = 0.0, dr2 = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double d0 = Fn[r] - st->F[r], d1 = Fn[4 + r] - st->F[4 + r], d2 = Fn[8 + r] - st->F[8 + r], d3 = Fn[12 + r] - st->F[12 + r];
      const double m = d0 * cx + d1 * cy + d2 * cz + d3;
      mv2 += m * m;
      dr2 += d0 * d0 + d1 * d1 + d2 * d2;
    }
    const float move = (float)(fast_sqrt(mv2) + fast_sqrt(dr2) * (double)st->src_r);
    st->last_move = move;
    if (move < st->cert_thr && st->cert_mode == 0) {
      st->cert_mode = 1;
      if (st->host_cert != nullptr) __hip_atomic_store(st->host_cert, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) st->F[i] = Fn[i];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) st->Ff[4 * r + c] = (float)Fn[4 * c + r];
  if (st->use_reciprocal) {
    // inverse of the affine part by the adjugate (F is rigid unless the caller's guess was not)
    const double a = Fn[0], b = Fn[4], c = Fn[8], d = Fn[1], e = Fn[5], f = Fn[9], g = Fn[2], h = Fn[6], i = Fn[10];
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    const double id = 1.0 / det;
    const double M[9] = {(e * i - f * h) * id, (c * h - b * i) * id, (b * f - c * e) * id,
                         (f * g - d * i) * id, (a * i - c * g) * id, (c * d - a * f) * id,
                         (d * h - e * g) * id, (b * g - a * h) * id, (a * e - b * d) * id};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      st->Finv[4 * r + 0] = (float)M[3 * r]; st->Finv[4 * r + 1] = (float)M[3 * r + 1]; st->Finv[4 * r + 2] = (float)M[3 * r + 2];
      st->Finv[4 * r + 3] = (float)(-(M[3 * r] * Fn[12] + M[3 * r + 1] * Fn[13] + M[3 * r + 2] * Fn[14]));
    }
  }
  const int iterations = ++st->iterations;

  // DefaultConvergenceCriteria::hasConverged (uPCL) with the thresholds wired at icp_mod.hpp:164-168
  st->state = OPE_CONV_NOT_CONVERGED;
  int conv = 0;
  if (iterations >= st->max_iterations) {
    if (!st->failure_after_max_iter) { st->state = OPE_CONV_ITERATIONS; conv = 1; }
    st->converged = conv;
    st->done = 1;
    return;
  }
  const double cos_angle = 0.5 * ((double)Tf[0] + (double)Tf[5] + (double)Tf[10] - 1.0);
  const double tr2 = (double)Tf[12] * Tf[12] + (double)Tf[13] * Tf[13] + (double)Tf[14] * Tf[14];
  if (cos_angle >= st->rotation_threshold && tr2 <= st->translation_threshold) {
    st->state = OPE_CONV_TRANSFORM;
    conv = 1;
  } else {
    st->cur_mse = S[16] / n;
    const double diff = fabs(st->cur_mse - st->prev_mse);
    if (diff < st->mse_threshold_absolute) { st->state = OPE_CONV_ABS_MSE; conv = 1; }
    else if (diff / st->prev_mse < st->mse_threshold_relative) { st->state = OPE_CONV_REL_MSE; conv = 1; }
    else st->prev_mse = st->cur_mse;
  }
  st->converged = conv;
  st->done = conv;
}

// The update lane works on an LDS copy of the state: its ~60 dependent accesses then cost LDS
// latency instead of one L2 round trip each (the global version took 18 us of a 22 us launch).
__device__ __forceinline__ void state_to_lds(IcpState *dst, const IcpState *src) {
  constexpr int kWords = (int)(sizeof(IcpState) / 4);
  static_assert(sizeof(IcpState) % 4 == 0, "IcpState must be a whole number of dwords");
  for (int i = threadIdx.x; i < kWords; i += blockDim.x)
    reinterpret_cast<uint32_t *>(dst)[i] = reinterpret_cast<const uint32_t *>(src)[i];
}

// Stand-alone TransformationEstimationSVD on n given pairs (packed xyz): block b of nb (256 lanes) adds the 17 sums about the first
// source point over the pairs b * 256 + lane, + nb * 256, ...; partials [17][nb].  The single launch (pairs_sums_kernel) and the
// segmented one of the batched correspondence aligner run these same instructions.
__device__ __forceinline__ void pairs_sums_block(const float *__restrict__ src, const float *__restrict__ tgt, uint32_t n, uint32_t b,
                                                 uint32_t nb, double *__restrict__ partials) {
  __shared__ double s_red[4][kNumSums];
  const float px = src[0], py = src[1], pz = src[2];
  double acc[kNumSums];
#pragma unroll
  for (int k = 0; k < kNumSums; ++k) acc[k] = 0.0;
  for (uint32_t i = b * 256 + threadIdx.x; i < n; i += nb * 256) {
    const double sx = (double)src[3 * i] - px, sy = (double)src[3 * i + 1] - py, sz = (double)src[3 * i + 2] - pz;
    const double tx = (double)tgt[3 * i] - px, ty = (double)tgt[3 * i + 1] - py, tz = (double)tgt[3 * i + 2] - pz;
    acc[0] += 1.0;
    acc[1] += sx; acc[2] += sy; acc[3] += sz;
    acc[4] += tx; acc[5] += ty; acc[6] += tz;
    acc[7] += tx * sx; acc[8] += tx * sy; acc[9] += tx * sz;
    acc[10] += ty * sx; acc[11] += ty * sy; acc[12] += ty * sz;
    acc[13] += tz * sx; acc[14] += tz * sy; acc[15] += tz * sz;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kNumSums; ++k) {
    const double v = wave_sum(acc[k]);
    if (lane == 0) s_red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < kNumSums)
    partials[threadIdx.x * nb + b] = s_red[0][threadIdx.x] + s_red[1][threadIdx.x] + s_red[2][threadIdx.x] + s_red[3][threadIdx.x];
}

// ... and the lane that adds the partials in block order and fits Umeyama (one wave)
__device__ __forceinline__ void pairs_umeyama_block(const double *__restrict__ partials, int nblocks, const float *__restrict__ src,
                                                    float *__restrict__ out_T) {
  __shared__ double s_S[kNumSums];
  if (threadIdx.x < kNumSums) {
    double v = 0.0;
    for (int b = 0; b < nblocks; ++b) v += partials[threadIdx.x * nblocks + b];
    s_S[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double pivot[3] = {(double)src[0], (double)src[1], (double)src[2]};
    double T[16];
    umeyama_from_sums(s_S, pivot, T);
#pragma unroll
    for (int i = 0; i < 16; ++i) out_T[i] = (float)T[i];
  }
}

}  // namespace ope
