// object_segmentation_plane.hpp — DetectAndLocalize's ObjectSegmentationPlane (objectsegmentationplane.cpp) on the device:
//
//     ope::ObjectSegmentationPlane objSegPlane;
//     bool isPlane = objSegPlane.getSegmentedObjectsOnPlane(cloudTargetFiltered, cloudClusterVector, cloudPlane);   // rosinterface.cpp:213
//
// getSegmentedObjectsOnPlane keeps the reference's signature and return values.  Steps 2-7 (:124-235) are one ope_tabletop_segment
// call on the uploaded frame, step 8 (getClusters, :239) is ope_euclidean_clusters_cloud on the non-plane cloud it left on the
// device; only index lists come back, and the output clouds of a HOST frame are gathered on the host from the input through
// them, so every field of the point type is carried.  A DEVICE frame with a colour payload hands it on to the clusters.  The members the reference exposes
// one by one (getPlaneIndicesAndCoeffSAC, getPlaneAndNonPlaneCloud, getClusters, getProjectedCloud) are here too, written
// with the façade's classes as the reference writes them with PCL's.  No ConvexHull: the reference uses the hull only through
// getMinMax3D, and the extremes of a planar set are attained at its hull's vertices.
#pragma once

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "pcl_compat.hpp"

namespace ope {

class ObjectSegmentationPlane {
 public:
  typedef compat::PointXYZRGB PointTObj;
  typedef compat::PointCloud<PointTObj> Cloud;

  void setSeed(uint64_t s) { seed_ = s; }
  const ope_tabletop_result &lastResult() const { return last_; }
  // getSegmentedObjectsExceptPlane's last peel: the planes' inlier counts in peeling order, and the call's result
  const std::vector<int32_t> &lastPeelCounts() const { return peelCounts_; }
  const ope_peel_result &lastPeel() const { return lastPeel_; }
  // getFiltered's limits.  The default is DetectAndLocalize's literals (objectsegmentationplane.cpp:17: -0.5 0.5, -0.5 0.3, 0.5 1.6);
  // BuildModel's file has -0.4 0.6, -0.5 0.5, 0.7 1.4 (BuildModel objectsegmentationplane.cpp:17).
  void setFilterLimits(float p_minX, float p_maxX, float p_minY, float p_maxY, float p_minZ, float p_maxZ) {
    filterLo_[0] = p_minX; filterLo_[1] = p_minY; filterLo_[2] = p_minZ;
    filterHi_[0] = p_maxX; filterHi_[1] = p_maxY; filterHi_[2] = p_maxZ;
  }

  // :8-33: the fixed pass-through (the reference's down-sampling after it is commented out)
  Cloud::Ptr getFiltered(Cloud::Ptr p_cloudInput) {
    Cloud::Ptr cloudOutput(new Cloud);
    ope_ctx *ctx = compat::default_context();
    if (!ctx || !p_cloudInput || p_cloudInput->empty()) return cloudOutput;
    auto frame = compat::upload(*p_cloudInput, false);
    std::vector<int32_t> idx(p_cloudInput->size());
    size_t n = 0;
    if (!frame->h || ope_pass_through(ctx, frame->h, filterLo_, filterHi_, idx.data(), &n) != OPE_OK) { compat::log_error("getFiltered", ctx); return cloudOutput; }
    cloudOutput->points.resize(n);
    for (size_t j = 0; j < n; ++j) cloudOutput->points[j] = p_cloudInput->points[(size_t)idx[j]];
    cloudOutput->width = (uint32_t)n;
    cloudOutput->height = 1;
    cloudOutput->is_dense = true;
    return cloudOutput;
  }

  // objectsegmentationplane.cpp:36-55
  bool getPlaneIndicesAndCoeffSAC(Cloud::Ptr p_cloudInput, compat::PointIndices::Ptr p_indices, compat::ModelCoefficients::Ptr p_modelCoeff) {
    sacSeg.setOptimizeCoefficients(true);
    sacSeg.setInputCloud(p_cloudInput);
    sacSeg.setModelType(compat::SACMODEL_PLANE);
    sacSeg.setMethodType(compat::SAC_RANSAC);
    sacSeg.setDistanceThreshold(0.01);
    sacSeg.setAxis(compat::Vector3f(0.0, 0.0, 1.0));
    sacSeg.setEpsAngle(10.0f * (3.14 / 180.0f));
    sacSeg.setSeed(seed_);
    sacSeg.segment(*p_indices, *p_modelCoeff);
    return p_modelCoeff->values.size() != 0;
  }

  // :58-71
  void getPlaneAndNonPlaneCloud(Cloud::Ptr p_cloudInput, compat::PointIndices::Ptr p_indices, Cloud::Ptr p_cloudPlane, Cloud::Ptr p_cloudNotPlane) {
    extractIndices.setInputCloud(p_cloudInput);
    extractIndices.setIndices(p_indices);
    extractIndices.setNegative(false);
    extractIndices.filter(*p_cloudPlane);
    extractIndices.setNegative(true);
    extractIndices.filter(*p_cloudNotPlane);
  }

  // :74-90
  std::vector<compat::PointIndices> getClusters(Cloud::Ptr p_cloudInput) {
    compat::search::KdTree<PointTObj>::Ptr kdTree(new compat::search::KdTree<PointTObj>);
    std::vector<compat::PointIndices> clusterIndices;
    euclideanClustExtraction.setInputCloud(p_cloudInput);
    euclideanClustExtraction.setSearchMethod(kdTree);
    euclideanClustExtraction.setClusterTolerance(0.05);
    euclideanClustExtraction.setMinClusterSize(300);
    euclideanClustExtraction.setMaxClusterSize(1e5);
    euclideanClustExtraction.extract(clusterIndices);
    return clusterIndices;
  }

  // :95-107
  Cloud::Ptr getProjectedCloud(Cloud::Ptr p_cloudInput, compat::PointIndices::Ptr p_indices, compat::ModelCoefficients::Ptr p_modelCoeff) {
    Cloud::Ptr cloudOutput(new Cloud);
    compat::ProjectInliers<PointTObj> projectInliers;
    projectInliers.setInputCloud(p_cloudInput);
    projectInliers.setModelType(compat::SACMODEL_PLANE);
    projectInliers.setIndices(p_indices);
    projectInliers.setModelCoefficients(p_modelCoeff);
    projectInliers.filter(*cloudOutput);
    return cloudOutput;
  }

  // :122-282.  false: no plane (first or second fit); the input is handed back as cluster 0, as the reference does.
  bool getSegmentedObjectsOnPlane(Cloud::Ptr p_cloudInput, std::vector<Cloud::Ptr> &cloudClusterVector, Cloud::Ptr &p_cloudPlane) {
    p_cloudPlane = Cloud::Ptr(new Cloud);
    last_ = ope_tabletop_result{};
    last_.status = OPE_TABLETOP_NO_PLANE_FIRST;
    auto hand_back = [&]() {   // copyPointCloud(*cloudFiltered, *cloudClusterVector.at(0)) (:157, :230)
      if (cloudClusterVector.empty()) cloudClusterVector.push_back(Cloud::Ptr(new Cloud));
      *cloudClusterVector[0] = *p_cloudInput;
      return false;
    };
    ope_ctx *ctx = compat::default_context();
    if (!ctx || !p_cloudInput) return p_cloudInput ? hand_back() : false;
    auto frame = compat::upload(*p_cloudInput, false);
    if (!frame->h) return hand_back();
    // the output clouds are gathered from the input, so every field of the point type (the colour) is carried
    return segmentDeviceFrame(ctx, frame->h, p_cloudInput->size(), [&](size_t i) { return p_cloudInput->points[i]; }, hand_back,
                              cloudClusterVector, p_cloudPlane);
  }

  // The same for a frame that is already on the device (DataGrabber::rgbd2PclDevice: converted from the depth image and cropped
  // there): the frame is not uploaded.  The host clouds the reference's signature asks for are built from ONE download of the
  // frame's xyz (12 B per point; the device clusters are in deviceClusters() for a caller that needs no host clouds), white like
  // DataGrabber::rgbd2Pcl's points (datagrabber.cpp:102-106).  false without a plane: cluster 0 is the frame.
  // A frame that carries colours (the coloured rgbd2PclDevice): the device clusters carry them too, and every host cloud takes
  // its colours from one ope_cloud_download_rgb of the device cloud it mirrors (the frame's own when it is handed back).
  bool getSegmentedObjectsOnPlane(const compat::CloudHandle &p_frame, std::vector<Cloud::Ptr> &cloudClusterVector, Cloud::Ptr &p_cloudPlane) {
    p_cloudPlane = Cloud::Ptr(new Cloud);
    last_ = ope_tabletop_result{};
    last_.status = OPE_TABLETOP_NO_PLANE_FIRST;
    ope_ctx *ctx = compat::default_context();
    if (!ctx || !p_frame.h) return false;
    const size_t n = ope_cloud_size(p_frame.h);
    std::vector<float> xyz(3 * n + 3);
    if (ope_cloud_download(ctx, p_frame.h, xyz.data()) != OPE_OK) { compat::log_error("getSegmentedObjectsOnPlane", ctx); return false; }
    const bool coloured = ope_cloud_has_rgb(p_frame.h) != 0;
    std::vector<uint32_t> frameRgb;   // fetched only when the frame itself is handed back
    auto point = [&](size_t i) {
      const uint32_t white = 0x00ffffffu;
      PointTObj q;
      q.x = xyz[3 * i]; q.y = xyz[3 * i + 1]; q.z = xyz[3 * i + 2];
      std::memcpy(&q.rgb, frameRgb.empty() ? &white : &frameRgb[i], 4);
      return q;
    };
    auto hand_back = [&]() {
      if (cloudClusterVector.empty()) cloudClusterVector.push_back(Cloud::Ptr(new Cloud));
      Cloud &out = *cloudClusterVector[0];
      if (coloured && n) {
        frameRgb.resize(n);
        if (ope_cloud_download_rgb(ctx, p_frame.h, frameRgb.data()) != OPE_OK) { compat::log_error("getSegmentedObjectsOnPlane", ctx); frameRgb.clear(); }
      }
      out.points.resize(n);
      for (size_t i = 0; i < n; ++i) out.points[i] = point(i);
      out.width = (uint32_t)n;
      out.height = 1;
      out.is_dense = true;
      return false;
    };
    return segmentDeviceFrame(ctx, p_frame.h, n, point, hand_back, cloudClusterVector, p_cloudPlane);
  }

  // :286-358.  The clusters of what is left when the planes are peeled off the cropped frame; deviceClusters() holds them as they
  // were left on the device.  The host clouds are gathered from the input through the index lists, so every field of the point
  // type (the colour) is carried.  No .pcd file is written: the reference's savePCDFile per cluster (:342-348) is a debugging
  // leftover with a path of its author's machine.
  std::vector<Cloud::Ptr> getSegmentedObjectsExceptPlane(Cloud::Ptr p_cloudInput) {
    std::vector<Cloud::Ptr> cloudClusterVector;
    resetPeel();
    ope_ctx *ctx = compat::default_context();
    if (!ctx || !p_cloudInput) return cloudClusterVector;
    auto frame = compat::upload(*p_cloudInput, false);
    if (!frame->h) { deviceFailed_ = true; return cloudClusterVector; }
    exceptPlaneDeviceFrame(ctx, frame->h, p_cloudInput->size(), [&](size_t i) { return p_cloudInput->points[i]; }, cloudClusterVector);
    return cloudClusterVector;
  }

  // The same for a frame that is already on the device: it is not uploaded.  The host clouds are built from ONE download of the
  // frame's xyz, white unless the frame carries colours (then each takes them from the device cluster it mirrors).
  std::vector<Cloud::Ptr> getSegmentedObjectsExceptPlane(const compat::CloudHandle &p_frame) {
    std::vector<Cloud::Ptr> cloudClusterVector;
    resetPeel();
    ope_ctx *ctx = compat::default_context();
    if (!ctx || !p_frame.h) return cloudClusterVector;
    const size_t n = ope_cloud_size(p_frame.h);
    std::vector<float> xyz(3 * n + 3);
    if (ope_cloud_download(ctx, p_frame.h, xyz.data()) != OPE_OK) {
      compat::log_error("getSegmentedObjectsExceptPlane", ctx);
      deviceFailed_ = true;
      return cloudClusterVector;
    }
    auto point = [&](size_t i) {
      const uint32_t white = 0x00ffffffu;
      PointTObj q;
      q.x = xyz[3 * i]; q.y = xyz[3 * i + 1]; q.z = xyz[3 * i + 2];
      std::memcpy(&q.rgb, &white, 4);
      return q;
    };
    exceptPlaneDeviceFrame(ctx, p_frame.h, n, point, cloudClusterVector);
    return cloudClusterVector;
  }

  // The same without any host cloud: only deviceClusters() is filled (BuildModel's scan loop hands cluster 0 straight to the
  // registration).  false without a plane, or when a device call failed (deviceFailed() tells the two apart); true with
  // deviceClusters() empty when nothing on the plane is a cluster.
  bool segmentOnDevice(const compat::CloudHandle &p_frame) {
    last_ = ope_tabletop_result{};
    last_.status = OPE_TABLETOP_NO_PLANE_FIRST;
    deviceClusters_.clear();
    deviceFailed_ = false;
    ope_ctx *ctx = compat::default_context();
    if (!ctx || !p_frame.h) { deviceFailed_ = true; return false; }
    compat::CloudHandle plane;
    return runOnDevice(ctx, p_frame.h, plane, nullptr, nullptr, nullptr, nullptr) == 0 && !deviceFailed_;
  }
  // the last call ended because a device call failed (its message is on stderr), not because the frame has no plane
  bool deviceFailed() const { return deviceFailed_; }

  // the clusters of the last successful call as they were left on the device (for ope_final_pose_batch / ope_track_pose without an upload)
  const std::vector<std::shared_ptr<compat::CloudHandle>> &deviceClusters() const { return deviceClusters_; }

 private:
  void resetPeel() {
    lastPeel_ = ope_peel_result{};
    peelCounts_.clear();
    deviceClusters_.clear();
    deviceFailed_ = false;
  }

  // getSegmentedObjectsExceptPlane on a frame of n points that is on the device: the crop (:292), the peel (:296-319) and
  // getClusters (:324), each handing a device cloud to the next; only index lists come back.  point(i): the host point of frame
  // index i.  A failed device call sets deviceFailed_ and leaves no clusters.
  template <class PointAt>
  void exceptPlaneDeviceFrame(ope_ctx *ctx, const ope_cloud *frame, size_t n, PointAt point, std::vector<Cloud::Ptr> &cloudClusterVector) {
    auto fail = [&]() { compat::log_error("getSegmentedObjectsExceptPlane", ctx); deviceFailed_ = true; };
    compat::CloudHandle filtered, rest;
    std::vector<int32_t> cropIdx(n + 1), restIdx;
    size_t nCrop = 0;
    if (ope_pass_through_cloud(ctx, frame, filterLo_, filterHi_, &filtered.h, cropIdx.data(), &nCrop) != OPE_OK) return fail();
    ope_plane_params p;
    ope_plane_default_params(&p);
    p.seed = seed_;
    const size_t capPlanes = 64;   // (more planes than this are peeled all the same; only their counts are not kept)
    peelCounts_.assign(capPlanes, 0);
    restIdx.assign(nCrop + 1, 0);
    if (ope_plane_peel(ctx, filtered.h, &p, nullptr, capPlanes, nullptr, peelCounts_.data(), nullptr, nullptr, restIdx.data(), &rest.h, &lastPeel_) !=
        OPE_OK) {
      peelCounts_.clear();
      return fail();
    }
    peelCounts_.resize(std::min<size_t>((size_t)lastPeel_.n_planes, capPlanes));
    const size_t m = (size_t)lastPeel_.n_rest;
    ope_cluster_params cp;
    ope_cluster_default_params(&cp);
    std::vector<ope_cloud *> clouds(m + 1, nullptr);
    std::vector<int32_t> idx(m + 1, 0), off(m + 2, 0);
    size_t k = 0;
    if (ope_euclidean_clusters_cloud(ctx, rest.h, &cp, m, &k, clouds.data(), idx.data(), off.data()) != OPE_OK) return fail();
    std::vector<uint32_t> rgb;
    for (size_t c = 0; c < k && c < m; ++c) {
      auto h = std::make_shared<compat::CloudHandle>();
      h->h = clouds[c];
      deviceClusters_.push_back(h);
      // the cluster's points by index (:330-337), through remainder and crop back to the frame
      const size_t cnt = (size_t)(off[c + 1] - off[c]);
      Cloud::Ptr cloudCluster(new Cloud);
      cloudCluster->points.resize(cnt);
      for (size_t j = 0; j < cnt; ++j) cloudCluster->points[j] = point((size_t)cropIdx[(size_t)restIdx[(size_t)idx[(size_t)off[c] + j]]]);
      if (cnt && ope_cloud_has_rgb(h->h)) {
        rgb.resize(cnt);
        if (ope_cloud_download_rgb(ctx, h->h, rgb.data()) == OPE_OK)
          for (size_t j = 0; j < cnt; ++j) std::memcpy(&cloudCluster->points[j].rgb, &rgb[j], 4);
        else compat::log_error("getSegmentedObjectsExceptPlane", ctx);
      }
      cloudCluster->width = (uint32_t)cnt;
      cloudCluster->height = 1;
      cloudCluster->is_dense = true;
      cloudClusterVector.push_back(cloudCluster);
    }
  }

  // Steps 2-8 on a frame of n points that is on the device.  point(i): the host point of frame index i, from which the output
  // clouds are gathered; hand_back(): what is returned when there is no plane.
  template <class PointAt, class HandBack>
  bool segmentDeviceFrame(ope_ctx *ctx, const ope_cloud *frame, size_t n, PointAt point, HandBack hand_back,
                          std::vector<Cloud::Ptr> &cloudClusterVector, Cloud::Ptr &p_cloudPlane) {
    compat::CloudHandle plane;
    std::vector<int32_t> planeIdx(n + 1), notPlaneIdx(n + 1), idx, off;
    deviceFailed_ = false;
    const int rc = runOnDevice(ctx, frame, plane, planeIdx.data(), notPlaneIdx.data(), &idx, &off);
    if (rc != 0) return hand_back();
    // dev: the device cloud `out` mirrors; when it carries colours they overwrite the gathered ones (one download per cloud)
    std::vector<uint32_t> rgb;
    auto gather = [&](Cloud &out, const int32_t *map, const int32_t *idx, size_t m, const ope_cloud *dev) {
      out.points.resize(m);
      for (size_t j = 0; j < m; ++j) out.points[j] = point((size_t)map[idx ? idx[j] : (int32_t)j]);
      if (dev && m && ope_cloud_has_rgb(dev)) {
        rgb.resize(m);
        if (ope_cloud_download_rgb(ctx, dev, rgb.data()) == OPE_OK)
          for (size_t j = 0; j < m; ++j) std::memcpy(&out.points[j].rgb, &rgb[j], 4);
        else compat::log_error("getSegmentedObjectsOnPlane", ctx);
      }
      out.width = (uint32_t)m;
      out.height = 1;
      out.is_dense = true;
    };
    gather(*p_cloudPlane, planeIdx.data(), nullptr, (size_t)last_.n_plane, plane.h);   // copyPointCloud(*cloudplane, *p_cloudPlane) (:235)
    // each cluster's points by index (:247-277)
    for (size_t c = 0; !deviceFailed_ && c < deviceClusters_.size(); ++c) {
      Cloud::Ptr cloudCluster(new Cloud);
      gather(*cloudCluster, notPlaneIdx.data(), idx.data() + off[c], (size_t)(off[c + 1] - off[c]), deviceClusters_[c]->h);
      cloudClusterVector.push_back(cloudCluster);
    }
    return true;
  }

  // Steps 2-7 (ope_tabletop_segment, the estimator's seed) and step 8 (getClusters, :239: ope_euclidean_clusters_cloud on the
  // non-plane cloud) on a device frame: deviceClusters_ is filled, `plane` receives the plane cloud.  planeIdx / notPlaneIdx (room
  // for every point of the frame) and idx / off (the clusters' points as indices into the non-plane cloud) are optional.
  // 0: a plane (a failed clustering call leaves no clusters and sets deviceFailed_); 1: no plane; -1: the segmentation call failed.
  int runOnDevice(ope_ctx *ctx, const ope_cloud *frame, compat::CloudHandle &plane, int32_t *planeIdx, int32_t *notPlaneIdx,
                  std::vector<int32_t> *idx, std::vector<int32_t> *off) {
    ope_plane_params p;
    ope_plane_default_params(&p);
    p.seed = seed_;
    compat::CloudHandle notPlane;
    if (ope_tabletop_segment(ctx, frame, &p, &last_, &plane.h, &notPlane.h, nullptr, planeIdx, notPlaneIdx) != OPE_OK) {
      compat::log_error("getSegmentedObjectsOnPlane", ctx);
      deviceFailed_ = true;
      return -1;
    }
    if (last_.status != OPE_TABLETOP_OK) return 1;
    const size_t m = (size_t)last_.n_not_plane;
    ope_cluster_params cp;
    ope_cluster_default_params(&cp);
    std::vector<ope_cloud *> clouds(m + 1, nullptr);
    if (idx) idx->assign(m + 1, 0);
    if (off) off->assign(m + 2, 0);
    size_t k = 0;
    if (ope_euclidean_clusters_cloud(ctx, notPlane.h, &cp, m, &k, clouds.data(), idx ? idx->data() : nullptr, off ? off->data() : nullptr) != OPE_OK) {
      compat::log_error("getSegmentedObjectsOnPlane", ctx);
      deviceFailed_ = true;
      return 0;
    }
    deviceClusters_.clear();   // (kept until here: they are the clusters of the last call that got this far)
    for (size_t c = 0; c < k && c < m; ++c) {
      auto h = std::make_shared<compat::CloudHandle>();
      h->h = clouds[c];
      deviceClusters_.push_back(h);
    }
    return 0;
  }

  compat::SACSegmentation<PointTObj> sacSeg;
  compat::ExtractIndices<PointTObj> extractIndices;
  compat::EuclideanClusterExtraction<PointTObj> euclideanClustExtraction;
  uint64_t seed_ = 12345;
  ope_tabletop_result last_{};
  float filterLo_[3] = {-0.5f, -0.5f, 0.5f}, filterHi_[3] = {0.5f, 0.3f, 1.6f};
  ope_peel_result lastPeel_{};
  std::vector<int32_t> peelCounts_;
  bool deviceFailed_ = false;
  std::vector<std::shared_ptr<compat::CloudHandle>> deviceClusters_;
};

}  // namespace ope
