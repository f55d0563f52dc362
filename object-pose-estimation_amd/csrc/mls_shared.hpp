// mls_shared.hpp — what mls.hip (the two walks of moving least squares) hands to mls_upsample.hip (the voxel-grid upsampling).
#pragma once

#include "ope_internal.hpp"

namespace ope {

// what walk A leaves for walk B, per SORTED position
struct MlsPlane {
  double pt[3];   // the query projected on its plane
  double n[3];    // the plane's normal (smallest eigenvector)
};

constexpr int kMlsMaxOrder = 4, kMlsMaxCoeff = 15;

// pcl::MovingLeastSquares::MLSResult, per ORIGINAL index; written for the points the plane kernel flags (3 or more neighbours).  u and v
// are not stored: they are Eigen's unitOrthogonal (n) and n x v when kMlsRecAxes is set (mls_axes), and zero otherwise, as 1.7 leaves them.
enum : uint32_t { kMlsRecAxes = 1u, kMlsRecSolved = 2u };   // polynomial_fit and m >= nr_coeff; every Cholesky pivot was > 0 and finite
struct MlsRecord {
  double mean[3], n[3];
  double c[kMlsMaxCoeff];   // the Cholesky solution (the first nr_coeff entries) when kMlsRecAxes is set
  int32_t m;                // neighbours
  uint32_t flags;
  float curvature;
  uint32_t pad_;
};

// words of the statistics block
enum { kMlsMin = 0, kMlsMax = 4, kMlsFinite = 8, kMlsFit = 9, kMlsNeighbours = 10 /* 64 bits */, kMlsWords = 12 };

// Eigen's unitOrthogonal (3-vectors) of n, then u = n x v
__host__ __device__ __forceinline__ void mls_axes(double nx, double ny, double nz, double (&u)[3], double (&v)[3]) {
  if (fabs(nx) > fabs(nz) * 1e-12 || fabs(ny) > fabs(nz) * 1e-12) {
    const double invnm = 1.0 / sqrt(nx * nx + ny * ny);
    v[0] = -ny * invnm; v[1] = nx * invnm; v[2] = 0.0;
  } else {
    const double invnm = 1.0 / sqrt(ny * ny + nz * nz);
    v[0] = 0.0; v[1] = -nz * invnm; v[2] = ny * invnm;
  }
  u[0] = ny * v[2] - nz * v[1]; u[1] = nz * v[0] - nx * v[2]; u[2] = nx * v[1] - ny * v[0];
}

// mls.hip: walk A and walk B in record mode over `cloud` and its index.  d_flag (n + 1 words, zeroed by the caller) gets 1 under the
// original index of every point with 3 or more neighbours, d_rec its MLSResult; d_stats (kMlsWords, initialised by the caller) the
// neighbour total.  d_self: self_leaves of the index.  Two launches, each checked.
hipError_t mls_fit_records(ope_ctx *ctx, const ope_cloud *cloud, const ope_index *ix, const uint32_t *d_self, float r2, double sgp,
                           int polynomial_fit, int order, uint32_t *d_flag, MlsRecord *d_rec, uint32_t *d_stats);
// mls.hip: bounding box (order-preserving keys in d_stats + kMlsMin / kMlsMax) and count (kMlsFinite) of the finite flagged rows of pos
hipError_t mls_bbox(hipStream_t s, const float *d_pos, const uint32_t *d_flag, uint32_t n, uint32_t *d_stats);
// mls.hip: nrm_sorted[p] = nrm_out[perm[p]]
hipError_t mls_normals_gather(hipStream_t s, const float4 *d_nrm_out, const int32_t *d_perm, uint32_t n, float4 *d_nrm_sorted);

}  // namespace ope
