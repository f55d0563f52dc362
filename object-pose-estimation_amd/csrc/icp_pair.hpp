// icp_pair.hpp — what an ICP iteration does with ONE query, each rule stated once: where its search starts, how it is moved, its
// distance to a normal's line and the test after it, the two per-pair rejectors, and how a block writes its sums out.  Every one of these is
// a bit-exactness rule pinned to the reference (operation order, precision, quirks).  Callers: the tree and grid accumulate
// kernels, the fixed-pair kernel and the fitness kernel (icp_kernels.hip), the survivor sums of the global rejectors
// (global_rejectors.hip), the search and survivor passes of the batched kernel (icp_batch.hip).  Which call sites keep a rule on
// their own text, and why, is listed in DESIGN.md 4.24.  The walks, the scheduling of chunks and the sums (icp_sums.hpp) are not here.
#pragma once

#include "icp_sums.hpp"

namespace ope {

// With a finite setMaxCorrespondenceDistance the 1-NN search only has to see points that can survive the threshold test
// (correspondence_estimation_mod.hpp:171 rejects d2 > max_d2 afterwards anyway): it starts from the smallest float strictly
// above every admissible d2 instead of +inf, so far-off queries end at the first boxes.
__device__ __forceinline__ float pair_start_bound(double max_d2) {
  float best0 = INFINITY;
  if (max_d2 < 3.0e38) {
    float f = (float)max_d2;
    if ((double)f < max_d2) f = nextafterf(f, INFINITY);
    best0 = nextafterf(f, INFINITY);
  }
  return best0;
}

// The per-run constants of a launch live in LDS (F rows [0..11], pivot [12..14], start bound [15]) and are re-read where they are
// used, through this pointer: held in registers across the walks they were spilled to scratch, 13 dwords per lane and launch.
// (It keeps its LDS address space — through a generic pointer the reads became flat_loads — and the optimiser cannot see through it.)
__device__ __forceinline__ lds_cfloat_ptr pair_consts(const float *s_const) {
  lds_cfloat_ptr cst = (lds_cfloat_ptr)s_const;
  asm volatile("" : "+v"(cst));
  return cst;
}

// A query as the search sees it: the source point moved by the run's 3x4 fp32 rows (xform_row: the oracle's operation order,
// unfused) and its normal rotated by the same rows; s: the point as stored (w = its original index).
struct MovedQuery {
  float4 s;
  float x, y, z, nx, ny, nz;
};
// rows: r[0 .. 11], the LDS constants (pair_consts) or a pointer to the rows themselves
template <class R>
__device__ __forceinline__ void pair_move_point(R rows, const float4 s, float &x, float &y, float &z) {
  float F[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) F[k] = rows[k];
  x = xform_row(F + 0, s.x, s.y, s.z);
  y = xform_row(F + 4, s.x, s.y, s.z);
  z = xform_row(F + 8, s.x, s.y, s.z);
}
// query i of src; NRM: with its normal, if the cloud has any (else zero)
template <bool NRM, class R>
__device__ __forceinline__ MovedQuery pair_moved_query(R rows, const CloudView &src, uint32_t i) {
  float F[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) F[k] = rows[k];
  MovedQuery q;
  q.s = src.xyzw[i];
  pair_move_point((const float *)F, q.s, q.x, q.y, q.z);
  q.nx = 0.f; q.ny = 0.f; q.nz = 0.f;
  if (NRM && src.nrm != nullptr) {
    const float4 n = src.nrm[i];
    q.nx = rot_row(F + 0, n.x, n.y, n.z);
    q.ny = rot_row(F + 4, n.x, n.y, n.z);
    q.nz = rot_row(F + 8, n.x, n.y, n.z);
  }
  return q;
}

// Normal shooting (…normal_shooting_weighted.hpp:115-135): the squared distance of target point p to the line through the query
// (x, y, z) along its normal — the difference in float, the cross product in double.
__device__ __forceinline__ double pair_line_dist2(const float4 p, float x, float y, float z, float nx, float ny, float nz) {
  const double vx = (double)__fsub_rn(p.x, x), vy = (double)__fsub_rn(p.y, y), vz = (double)__fsub_rn(p.z, z);
  const double cx = (double)ny * vz - (double)nz * vy;
  const double cy = (double)nz * vx - (double)nx * vz;
  const double cz = (double)nx * vy - (double)ny * vx;
  return cx * cx + cy * cy + cz * cz;
}
// Whether the pick among the k nearest (count of them, the smallest squared line distance) gives a pair.
// quirk Q2: the SQUARED line distance is tested against the UNSQUARED max distance (:136)
__device__ __forceinline__ bool pair_ns_ok(int count, double min_dist, double max_dist_unsq) { return count > 0 && !(min_dist > max_dist_unsq); }

// The per-pair rejectors (correspondence_rejection_mod.h:368-391).  Surface normal: the dot product of the moved source normal and
// the target normal tn, in float, against the threshold.
__device__ __forceinline__ bool pair_passes_surface_normal(float nx, float ny, float nz, const float4 tn, double thr_sn) {
  const float score = __fadd_rn(__fadd_rn(__fmul_rn(nx, tn.x), __fmul_rn(ny, tn.y)), __fmul_rn(nz, tn.z));
  return (double)score > thr_sn;
}
// Self occlusion: the moved source normal against the direction from the moved point to the sensor at the origin; the squared
// length in float, everything after it in double.
__device__ __forceinline__ bool pair_passes_self_occlusion(float x, float y, float z, float nx, float ny, float nz, double thr_so) {
  const double sl = sqrt((double)__fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z)));
  const double score = (double)nx * (-(double)x / sl) + (double)ny * (-(double)y / sl) + (double)nz * (-(double)z / sl);
  return score > thr_so;
}

// wave rows (s_red[w][k]) -> the block's partial, in a fixed order, by threads 0 .. nsums - 1.  One-GPU runs keep one row per block
// and reduce the rows in a fixed tree (bit-reproducible for a launch geometry); sharded runs add straight into the sums the
// all-reduce takes next (S_atomic): one launch less per iteration, an addition order that varies from run to run (1e-16).
template <int WAVES>
__device__ __forceinline__ void pair_write_block_partial(const double (*s_red)[kNumSumsMax], int nsums, double *S_atomic, double *partials) {
  if ((int)threadIdx.x < nsums) {
    double v = 0.0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) v += s_red[w][threadIdx.x];
    if (S_atomic != nullptr) unsafeAtomicAdd(S_atomic + threadIdx.x, v);
    else partials[threadIdx.x * kAccMaxBlocks + blockIdx.x] = v;
  }
}

}  // namespace ope
