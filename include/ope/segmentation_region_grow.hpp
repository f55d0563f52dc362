// segmentation_region_grow.hpp — the reference's SegmentationRegionGrow (segmentationregiongrow.cpp, identical in BuildModel and
// DetectAndLocalize) on the device:
//
//     ope::SegmentationRegionGrow segRegGrow;
//     Cloud::Ptr last = segRegGrow.getSegmentRegGrow(cloudInput);     // the reference's return value (:80: the LAST cluster)
//     const auto &all = segRegGrow.getClusters();                     // every cluster, in pcl::RegionGrowing's order
//
// getSegmentRegGrow (:9-82): PassThrough on z over [0, 1.2], NormalEstimation with k = 30, pcl::RegionGrowing with 15 neighbours,
// 10 degrees, curvature threshold 1.0 and clusters of 500 to 1 000 000 points.  Here the crop is ope_pass_through_cloud and the
// rest one ope_region_grow_cloud call that estimates the normals itself; only index lists come back, and the host clouds are
// gathered from the input through them, so every field of the point type (the colour) is carried.  deviceClusters() holds the
// clusters as they were left on the device, normals attached.
// Two things the reference does are not reproduced.  It gathers each cluster from the UNCROPPED input with indices of the CROPPED
// cloud (:52), which picks unrelated points whenever the crop removes any: the clusters here are gathered from the cropped cloud.
// And it saves every cluster under a path of its author's machine (:66-72): no file is written.
// getSegmentRegGrowRgb (:85-151): PassThrough on z over [0, 1.1] and pcl::RegionGrowingRGB with distance threshold 0.1, point and
// region colour thresholds 10 and clusters of at least 700 points: the same crop and one ope_region_grow_rgb_cloud
// call.  The reference passes the crop as indices, so its clusters do index the input; here they are gathered through the crop,
// which is the same points.  getClusters(), deviceClusters() and the returned LAST cluster (:130) as above; lastRgbStats() is what
// the call did.  A frame that is already on the device must carry its colours.
#pragma once

#include <cfloat>
#include <cstring>
#include <memory>
#include <vector>

#include "pcl_compat.hpp"

namespace ope {

class SegmentationRegionGrow {
 public:
  typedef compat::PointXYZRGB PointTSeg;
  typedef compat::PointCloud<PointTSeg> Cloud;

  // every cluster of the last call, in seed order; the same on the device; what the call did
  const std::vector<Cloud::Ptr> &getClusters() const { return clusters_; }
  const std::vector<std::shared_ptr<compat::CloudHandle>> &deviceClusters() const { return deviceClusters_; }
  const ope_region_stats &lastStats() const { return stats_; }
  const ope_region_rgb_stats &lastRgbStats() const { return rgbStats_; }
  // points the z crop kept in the last call
  size_t lastCropSize() const { return nCrop_; }
  // the last call ended because a device call failed or refused (its message is on stderr), not because nothing is a cluster
  bool deviceFailed() const { return deviceFailed_; }
  // the reference's literals (:19, :25-36) unless changed
  ope_region_params &params() { return params_; }
  void setFilterLimitsZ(float lo, float hi) { zLo_ = lo; zHi_ = hi; }
  // the same for getSegmentRegGrowRgb (:94, :100-103)
  ope_region_rgb_params &rgbParams() { return rgbParams_; }
  void setFilterLimitsZRgb(float lo, float hi) { zLoRgb_ = lo; zHiRgb_ = hi; }

  SegmentationRegionGrow() { ope_region_default_params(&params_); ope_region_rgb_default_params(&rgbParams_); }

  // :9-82.  An empty cloud when there is no cluster.
  Cloud::Ptr getSegmentRegGrow(Cloud::Ptr p_cloudInput) {
    reset();
    ope_ctx *ctx = compat::default_context();
    if (!ctx || !p_cloudInput) { deviceFailed_ = !ctx; return Cloud::Ptr(new Cloud); }
    auto frame = compat::upload(*p_cloudInput, false);
    if (!frame->h) { deviceFailed_ = true; return Cloud::Ptr(new Cloud); }
    return run(ctx, frame->h, p_cloudInput->size(), [&](size_t i) { return p_cloudInput->points[i]; }, false);
  }

  // :85-151.  An empty cloud when there is no cluster.
  Cloud::Ptr getSegmentRegGrowRgb(Cloud::Ptr p_cloudInput) {
    reset();
    ope_ctx *ctx = compat::default_context();
    if (!ctx || !p_cloudInput) { deviceFailed_ = !ctx; return Cloud::Ptr(new Cloud); }
    auto frame = compat::upload(*p_cloudInput, false);
    std::vector<uint32_t> rgb(p_cloudInput->size() + 1);
    for (size_t i = 0; i < p_cloudInput->size(); ++i) std::memcpy(&rgb[i], &p_cloudInput->points[i].rgb, 4);
    if (!frame->h || ope_cloud_set_rgb(ctx, frame->h, rgb.data()) != OPE_OK) { deviceFailed_ = true; return Cloud::Ptr(new Cloud); }
    return run(ctx, frame->h, p_cloudInput->size(), [&](size_t i) { return p_cloudInput->points[i]; }, true);
  }

  // The same for a frame that is already on the device: it is not uploaded.  The host clouds are built from ONE download of the
  // frame's xyz, white unless the frame carries colours (then each takes them from the device cluster it mirrors).
  Cloud::Ptr getSegmentRegGrow(const compat::CloudHandle &p_frame) { return fromDevice(p_frame, false); }
  Cloud::Ptr getSegmentRegGrowRgb(const compat::CloudHandle &p_frame) { return fromDevice(p_frame, true); }

 private:
  Cloud::Ptr fromDevice(const compat::CloudHandle &p_frame, bool rgb) {
    reset();
    ope_ctx *ctx = compat::default_context();
    if (!ctx || !p_frame.h) { deviceFailed_ = true; return Cloud::Ptr(new Cloud); }
    const size_t n = ope_cloud_size(p_frame.h);
    std::vector<float> xyz(3 * n + 3);
    if (ope_cloud_download(ctx, p_frame.h, xyz.data()) != OPE_OK) {
      compat::log_error(rgb ? "getSegmentRegGrowRgb" : "getSegmentRegGrow", ctx);
      deviceFailed_ = true;
      return Cloud::Ptr(new Cloud);
    }
    auto point = [&](size_t i) {
      const uint32_t white = 0x00ffffffu;
      PointTSeg q;
      q.x = xyz[3 * i]; q.y = xyz[3 * i + 1]; q.z = xyz[3 * i + 2];
      std::memcpy(&q.rgb, &white, 4);
      return q;
    };
    return run(ctx, p_frame.h, n, point, rgb);
  }

  void reset() {
    clusters_.clear();
    deviceClusters_.clear();
    stats_ = ope_region_stats{};
    rgbStats_ = ope_region_rgb_stats{};
    nCrop_ = 0;
    deviceFailed_ = false;
  }

  // the crop (:17-20) and the region grow (:23-39) on a frame of n points that is on the device, each cluster gathered by index
  // (:47-56) through the crop back to the frame.  point(i): the host point of frame index i.  rgb: the crop and the region grow
  // of getSegmentRegGrowRgb (:92-106) instead.
  template <class PointAt> Cloud::Ptr run(ope_ctx *ctx, const ope_cloud *frame, size_t n, PointAt point, bool rgb) {
    Cloud::Ptr last(new Cloud);
    const char *who = rgb ? "getSegmentRegGrowRgb" : "getSegmentRegGrow";
    auto fail = [&]() { compat::log_error(who, ctx); deviceFailed_ = true; return last; };
    compat::CloudHandle filtered;
    std::vector<int32_t> cropIdx(n + 1);
    const float lo[3] = {-FLT_MAX, -FLT_MAX, rgb ? zLoRgb_ : zLo_}, hi[3] = {FLT_MAX, FLT_MAX, rgb ? zHiRgb_ : zHi_};
    if (ope_pass_through_cloud(ctx, frame, lo, hi, &filtered.h, cropIdx.data(), &nCrop_) != OPE_OK) return fail();
    const size_t m = nCrop_;
    std::vector<ope_cloud *> clouds(m + 1, nullptr);
    std::vector<int32_t> idx(m + 1, 0), off(m + 2, 0);
    size_t k = 0;
    const int rc = rgb ? ope_region_grow_rgb_cloud(ctx, filtered.h, &rgbParams_, m, &k, clouds.data(), idx.data(), off.data())
                       : ope_region_grow_cloud(ctx, filtered.h, &params_, nullptr, nullptr, m, &k, clouds.data(), idx.data(), off.data());
    if (rgb) ope_region_rgb_last_stats(ctx, &rgbStats_);
    else ope_region_last_stats(ctx, &stats_);
    if (rc != OPE_OK) return fail();
    std::vector<uint32_t> colours;
    for (size_t c = 0; c < k && c < m; ++c) {
      auto h = std::make_shared<compat::CloudHandle>();
      h->h = clouds[c];
      deviceClusters_.push_back(h);
      const size_t cnt = (size_t)(off[c + 1] - off[c]);
      Cloud::Ptr cloudCluster(new Cloud);
      cloudCluster->points.resize(cnt);
      for (size_t j = 0; j < cnt; ++j) cloudCluster->points[j] = point((size_t)cropIdx[(size_t)idx[(size_t)off[c] + j]]);
      if (cnt && ope_cloud_has_rgb(h->h)) {
        colours.resize(cnt);
        if (ope_cloud_download_rgb(ctx, h->h, colours.data()) == OPE_OK)
          for (size_t j = 0; j < cnt; ++j) std::memcpy(&cloudCluster->points[j].rgb, &colours[j], 4);
        else compat::log_error(who, ctx);
      }
      cloudCluster->width = (uint32_t)cnt;
      cloudCluster->height = 1;
      cloudCluster->is_dense = true;
      clusters_.push_back(cloudCluster);
    }
    if (!clusters_.empty()) *last = *clusters_.back();   // `*cloudClusterFirst = *cloudCluster` in every round (:63): the last one stays
    return last;
  }

  ope_region_params params_;
  ope_region_rgb_params rgbParams_;
  float zLo_ = 0.0f, zHi_ = 1.2f, zLoRgb_ = 0.0f, zHiRgb_ = 1.1f;
  std::vector<Cloud::Ptr> clusters_;
  std::vector<std::shared_ptr<compat::CloudHandle>> deviceClusters_;
  ope_region_stats stats_{};
  ope_region_rgb_stats rgbStats_{};
  size_t nCrop_ = 0;
  bool deviceFailed_ = false;
};

}  // namespace ope
