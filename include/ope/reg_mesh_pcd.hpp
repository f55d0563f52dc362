// reg_mesh_pcd.hpp — BuildModel's RegMeshPcd (BuildModel/include/regmeshpcd.h:27-49, src/regmeshpcd.cpp:8-271) on the
// façade: getIcp (stock point-to-point ICP), getIcpNormal (normals k = 12, normal shooting k = 20, surface-normal
// rejector, point-to-plane LM estimator, eps 1e-8 / 1e-8) and registerPointClouds (sequential accumulate-and-register).
// generateMeshCloud is generateMesh up to the cloud it hands to the triangulation (:275-303: MLS upsampling by voxel-grid dilation,
// then normals k = 20); the greedy triangulation and the VTK smoothing (:305-343) are sequential surface reconstruction, out of scope.
//
// Kept from the reference on purpose:
//   * p_maxCorrDist only reaches a stand-alone determineCorrespondences call whose result is discarded (:140-159); the ICP
//     object itself keeps PCL's default correspondence distance;
//   * cloudTemp aliases cloudVector[0] (:229): `*cloudTemp = *cloudAlignedIcp` overwrites the caller's first frame with the
//     accumulated cloud, pair after pair;
//   * the accumulated cloud is `aligned source + target` in that order (:254-258), colours carried along.
#pragma once

#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "pcl_compat.hpp"

namespace ope {

class RegMeshPcd {
 public:
  typedef compat::PointXYZRGB PointTReg;
  typedef compat::PointCloud<PointTReg> Cloud;
  typedef compat::PointXYZRGBNormal PN;
  typedef compat::PointCloud<PN> CloudN;

  // per-pair results, for callers that want more than the cloud
  struct Pair { compat::Matrix4f T; int iterations; bool converged; double fitness; };
  const std::vector<Pair> &pairs() const { return pairs_; }

  // :8-59  plain IterativeClosestPoint (stock icp.h in the reference)
  Cloud::Ptr getIcp(Cloud::Ptr p_cloudSource, Cloud::Ptr p_cloudTarget, float p_maxCorrDist, float p_ransacStatOutThresh, int p_maxIterations) {
    compat::IterativeClosestPoint<PointTReg, PointTReg> icp;
    icp.setInputSource(p_cloudSource);
    icp.setInputTarget(p_cloudTarget);
    icp.setMaxCorrespondenceDistance(p_maxCorrDist);                  // :23
    icp.setRANSACOutlierRejectionThreshold(p_ransacStatOutThresh);    // :26 (accepted; the reference's ICP never reads it)
    icp.setMaximumIterations(p_maxIterations);                        // :29
    icp.setTransformationEpsilon(1e-8);                               // :32
    icp.setEuclideanFitnessEpsilon(1e-8);                             // :35
    Cloud::Ptr cloudAligned(new Cloud);
    icp.align(*cloudAligned);
    std::printf("ICP converged with score: %g\n", icp.getFitnessScore());
    return cloudAligned;
  }

  // :63-206
  Cloud::Ptr getIcpNormal(Cloud::Ptr p_cloudSource, Cloud::Ptr p_cloudTarget, float p_maxCorrDist, float /*p_ransacStatOutThresh*/, int p_maxIterations) {
    CloudN::Ptr cloudSourceWithNormal = withNormals(p_cloudSource), cloudTargetWithNormal = withNormals(p_cloudTarget);   // :72-90
    typedef compat::registration::CorrespondenceEstimationNormalShooting<PN, PN, PN> NS;
    NS::Ptr corrEstNormShoot(new NS);
    corrEstNormShoot->setInputSource(cloudSourceWithNormal);
    corrEstNormShoot->setSourceNormals(cloudSourceWithNormal);
    corrEstNormShoot->setInputTarget(cloudTargetWithNormal);
    corrEstNormShoot->setKSearch(20);                                 // :144
    (void)p_maxCorrDist;   // :145 passes it to a stand-alone determineCorrespondences whose result is never used
    compat::registration::CorrespondenceRejectorSurfaceNormal::Ptr corrRejSurNorm(new compat::registration::CorrespondenceRejectorSurfaceNormal);
    corrRejSurNorm->initializeDataContainer<PN, PN>();
    corrRejSurNorm->setThreshold(corrRejThreshNormAngle);             // :158
    compat::registration::TransformationEstimationPointToPlane<PN, PN>::Ptr transfEstpointToPlane(
        new compat::registration::TransformationEstimationPointToPlane<PN, PN>);                                          // :162 (LM)
    compat::IterativeClosestPointWithNormals<PN, PN> icpNorm;
    icpNorm.setInputSource(cloudSourceWithNormal);
    icpNorm.setInputTarget(cloudTargetWithNormal);
    icpNorm.setMaximumIterations(p_maxIterations);                    // :179
    icpNorm.setTransformationEpsilon(1e-8);                           // :182
    icpNorm.setEuclideanFitnessEpsilon(1e-8);                         // :184
    icpNorm.setCorrespondenceEstimation(corrEstNormShoot);            // :187
    icpNorm.addCorrespondenceRejector(corrRejSurNorm);                // :190
    icpNorm.setTransformationEstimation(transfEstpointToPlane);       // :193
    CloudN cloudIcpNormal;
    icpNorm.align(cloudIcpNormal);                                    // :196
    const double score = icpNorm.getFitnessScore();
    std::printf("ICP converged with score: %g\n", score);            // :198
    const compat::Matrix4f transformIcpNormal = icpNorm.getFinalTransformation();
    pairs_.push_back(Pair{transformIcpNormal, icpNorm.getNumberOfIterations(), icpNorm.hasConverged(), score});
    Cloud::Ptr cloudAligned(new Cloud);
    compat::transformPointCloud(*p_cloudSource, *cloudAligned, transformIcpNormal);   // :203
    return cloudAligned;
  }

  // :210-271
  Cloud::Ptr registerPointClouds(std::vector<Cloud::Ptr> &cloudVector, float maxCorrDist, float corrRejThresh, int maxIter) {
    const float ransacStatOutThresh2 = 0.02f;   // :222
    corrRejThreshNormAngle = corrRejThresh;     // :227
    pairs_.clear();
    Cloud::Ptr out(new Cloud);
    if (cloudVector.empty()) return out;
    Cloud::Ptr cloudTemp = cloudVector[0];      // :229 (aliases the caller's first frame)
    for (size_t i = 0; i + 1 < cloudVector.size(); ++i) {
      std::printf("ICP between frame %zu and %zu\n", i, i + 1);
      Cloud::Ptr cloudSource = cloudTemp, cloudTarget = cloudVector[i + 1];
      Cloud::Ptr cloudAlignedIcp = getIcpNormal(cloudSource, cloudTarget, maxCorrDist, ransacStatOutThresh2, maxIter);   // :251
      for (const auto &p : cloudTarget->points) cloudAlignedIcp->push_back(p);                                           // :254  *aligned += *target
      *cloudTemp = *cloudAlignedIcp;                                                                                    // :258
    }
    *out = *cloudTemp;   // :266
    return out;
  }

  // :210-271 over frames that are on the device (ObjectSegmentationPlane::deviceClusters()): the same sequence through the C
  // ABI.  Normals (k = 12) are attached to the clouds as they come, the accumulated cloud is ope_cloud_concat (transform, append
  // and re-sort on the device; colours carried when every frame has them) and never leaves the device: one download of its
  // points and one of its colours at the end (white without colours).  The frames stay the caller's.  Empty on failure.
  Cloud::Ptr registerPointClouds(const std::vector<std::shared_ptr<compat::CloudHandle>> &cloudVector, float /*maxCorrDist*/, float corrRejThresh,
                                 int maxIter) {
    corrRejThreshNormAngle = corrRejThresh;     // :227
    pairs_.clear();
    Cloud::Ptr out(new Cloud);
    ope_ctx *ctx = compat::default_context();
    if (!ctx || cloudVector.empty()) return out;
    for (const auto &c : cloudVector)
      if (!c || !c->h) return out;
    ope_icp_params p;
    ope_icp_default_params(&p);
    p.max_iterations = maxIter;                          // :179
    p.transformation_epsilon = 1e-8;                     // :182
    p.euclidean_fitness_epsilon = 1e-8;                  // :184
    p.corr_mode = OPE_CORR_NORMAL_SHOOTING;              // :139-145,:187
    p.k_normal_shooting = 20;                            // :144
    p.use_surface_normal_rej = 1;                        // :148-158,:190
    p.surface_normal_thr = corrRejThresh;                // :158
    p.estimator = OPE_EST_POINT_TO_PLANE_LM;             // :162,:193
    const float vp[3] = {0.f, 0.f, 0.f};
    auto fail = [&](const char *where) { compat::log_error(where, ctx); return Cloud::Ptr(new Cloud); };
    std::shared_ptr<compat::CloudHandle> acc = cloudVector[0];
    for (size_t i = 0; i + 1 < cloudVector.size(); ++i) {
      std::printf("ICP between frame %zu and %zu\n", i, i + 1);
      ope_cloud *tgt = cloudVector[i + 1]->h;
      if (ope_normals(ctx, acc->h, 12, vp, nullptr, nullptr) != OPE_OK || ope_normals(ctx, tgt, 12, vp, nullptr, nullptr) != OPE_OK)   // :72-90
        return fail("registerPointClouds (normals)");
      compat::IndexHandle index;
      if (ope_index_build(ctx, tgt, nullptr, &index.h) != OPE_OK) return fail("registerPointClouds (index)");
      Pair pr{compat::Matrix4f::Identity(), 0, false, 0.0};
      ope_icp_result res;
      if (ope_icp_run(ctx, acc->h, index.h, nullptr, &p, pr.T.m, &res) != OPE_OK) return fail("registerPointClouds (icp)");              // :196
      if (ope_fitness(ctx, acc->h, index.h, pr.T.m, DBL_MAX, &pr.fitness, nullptr, nullptr) != OPE_OK) return fail("registerPointClouds (fitness)");
      std::printf("ICP converged with score: %g\n", pr.fitness);                                                                        // :198
      pr.iterations = res.iterations;
      pr.converged = res.converged != 0;
      pairs_.push_back(pr);
      auto next = std::make_shared<compat::CloudHandle>();
      if (ope_cloud_concat(ctx, acc->h, pr.T.m, tgt, &next->h) != OPE_OK) return fail("registerPointClouds (concat)");                   // :203, :254
      acc = next;
    }
    if (smoothRadius_ > 0.f) {   // :264-266 getSmooth(cloudTemp, radius): on the device, before the one download
      ope_mls_params mp;
      ope_mls_default_params(&mp);
      mp.radius = smoothRadius_;
      auto smooth = std::make_shared<compat::CloudHandle>();
      size_t kept = 0;
      if (ope_mls_smooth_cloud(ctx, acc->h, &mp, &smooth->h, nullptr, &kept) != OPE_OK) return fail("registerPointClouds (smooth)");
      acc = smooth;
    }
    const size_t n = ope_cloud_size(acc->h);
    std::vector<float> xyz(3 * n + 3);
    std::vector<uint32_t> rgb(n + 1, 0x00ffffffu);
    if (ope_cloud_download(ctx, acc->h, xyz.data()) != OPE_OK) return fail("registerPointClouds (download)");
    if (ope_cloud_has_rgb(acc->h) && ope_cloud_download_rgb(ctx, acc->h, rgb.data()) != OPE_OK) return fail("registerPointClouds (download)");
    out->points.resize(n);
    for (size_t k = 0; k < n; ++k) {
      PointTReg &q = out->points[k];
      q.x = xyz[3 * k]; q.y = xyz[3 * k + 1]; q.z = xyz[3 * k + 2];
      std::memcpy(&q.rgb, &rgb[k], 4);
    }
    out->width = (uint32_t)n;
    out->height = 1;
    out->is_dense = true;
    return out;
  }

  // :275-303  what generateMesh hands to the greedy triangulation: the cloud upsampled by MovingLeastSquares (order 4, radius 0.03,
  // VOXEL_GRID_DILATION with voxels of 0.002 and no dilation round) with the normals of NormalEstimation k = 20 on it.  On the device;
  // the result stays there (normals attached, w = curvature).  Null on failure.
  std::shared_ptr<compat::CloudHandle> generateMeshCloud(const std::shared_ptr<compat::CloudHandle> &p_cloud) {
    ope_ctx *ctx = compat::default_context();
    if (!ctx || !p_cloud || !p_cloud->h) return nullptr;
    ope_mls_upsample_params mp;
    ope_mls_upsample_default_params(&mp);
    mp.radius = 0.03;                 // :280
    mp.polynomial_fit = 1;            // :281
    mp.order = 4;                     // :282
    mp.voxel_size = 0.002f;           // :286
    auto up = std::make_shared<compat::CloudHandle>();
    size_t n = 0;
    if (ope_mls_upsample_cloud(ctx, p_cloud->h, &mp, &up->h, nullptr, 0, &n) != OPE_OK) { compat::log_error("generateMeshCloud (upsampling)", ctx); return nullptr; }
    const float vp[3] = {0.f, 0.f, 0.f};
    if (n && ope_normals(ctx, up->h, 20, vp, nullptr, nullptr) != OPE_OK) { compat::log_error("generateMeshCloud (normals)", ctx); return nullptr; }   // :291-298
    return up;
  }
  // the same from and to the host: the PointXYZRGBNormal cloud of concatenateFields (:303), rgb left at its default as there
  CloudN::Ptr generateMeshCloud(const compat::PointCloud<compat::PointXYZ>::Ptr &p_cloud) {
    CloudN::Ptr out(new CloudN);
    ope_ctx *ctx = compat::default_context();
    if (!ctx || !p_cloud || p_cloud->empty()) return out;
    const auto up = generateMeshCloud(compat::upload(*p_cloud, false));
    if (!up) return out;
    const size_t n = ope_cloud_size(up->h);
    if (n == 0) return out;
    std::vector<float> xyz(3 * n), nrm(3 * n), curv(n);
    if (ope_cloud_download(ctx, up->h, xyz.data()) != OPE_OK || ope_cloud_download_normals(ctx, up->h, nrm.data(), curv.data()) != OPE_OK) {
      compat::log_error("generateMeshCloud (download)", ctx);
      return out;
    }
    out->points.resize(n);
    for (size_t k = 0; k < n; ++k) {
      PN &q = out->points[k];
      q.x = xyz[3 * k]; q.y = xyz[3 * k + 1]; q.z = xyz[3 * k + 2];
      q.normal_x = nrm[3 * k]; q.normal_y = nrm[3 * k + 1]; q.normal_z = nrm[3 * k + 2];
      q.curvature = curv[k];
    }
    out->width = (uint32_t)n;
    out->height = 1;
    out->is_dense = true;
    return out;
  }

  // opt-in: the device overload of registerPointClouds smooths the finished model with this radius (0: off, the default)
  void setSmoothRadius(float radius) { smoothRadius_ = radius; }

 private:
  float smoothRadius_ = 0.f;
  // NormalEstimation<PointXYZRGB, PointXYZRGBNormal>(k = 12), then copyPointCloud of xyz / rgb into it (:72-90)
  static CloudN::Ptr withNormals(const Cloud::Ptr &c) {
    CloudN::Ptr n(new CloudN);
    compat::NormalEstimation<PointTReg, PN> normEst;
    normEst.setSearchMethod(std::make_shared<compat::search::KdTree<PointTReg>>());
    normEst.setKSearch(12);
    normEst.setInputCloud(c);
    normEst.compute(*n);
    for (size_t i = 0; i < c->size() && i < n->size(); ++i) {
      (*n)[i].x = (*c)[i].x; (*n)[i].y = (*c)[i].y; (*n)[i].z = (*c)[i].z; (*n)[i].rgb = (*c)[i].rgb;
    }
    return n;
  }

  float corrRejThreshNormAngle = 0.7f;
  std::vector<Pair> pairs_;
};

}  // namespace ope
