// object_tracker.hpp — the per-frame policy of DetectAndLocalize (rosinterface.cpp:226-313) around one ope::PoseEstimator:
//
//     ope::ObjectTracker tracker(cloudSourceOriginal);                   // rosinterface.cpp:80 loads the model
//     pose = tracker.localize(cloudClusterVector, fitnessScore, alignedStrength);   // once per camera frame
//
//   * no clusters: nothing runs, the pose and cloudSource stay as they are (:220);
//   * the first frame: the candidate loop from the original model (PoseEstimator::estimateFinalPoseCandidates);
//   * later frames: ope_track_pose — the centroid gate on the device, then estimateFinalPose(cloudSource, the first non-empty
//     cluster within 5 cm), or the candidate loop again when the last distance exceeds 5 cm.  The estimator is then left as those
//     calls would leave it (PoseEstimator::replayTrackedFrame / replayCandidates).  The aligned model stays on the device between
//     frames, so a gated frame uploads the clusters only.
// localizeLoop() is the same policy written out as the reference writes it: host compute3DCentroid and estimateFinalPose.  It is
// what localize() falls back to when ope_track_pose refuses the clouds, and when cloudSource is not the estimator's alignedSource
// (a first frame whose last visited cluster was empty) while the coarse stage would be skipped.
#pragma once

#include <cmath>
#include <memory>
#include <vector>

#include "pose_estimator.hpp"

namespace ope {

class ObjectTracker {
 public:
  typedef PoseEstimator::Cloud Cloud;
  typedef PoseEstimator::Matrix4f Matrix4f;
  enum Branch { NO_CLUSTERS = 0, GATED = 1, REALIGN = 2, NOTHING = 3, FIRST = 5 };

  explicit ObjectTracker(const Cloud &model) : cloudSourceOriginal(new Cloud(model)), cloudSource(new Cloud(model)) {}

  PoseEstimator &estimator() { return poseEstimator; }
  const Cloud &source() const { return *cloudSource; }
  Matrix4f pose() const { return pose_; }
  int lastBranch() const { return branch_; }
  int lastSelected() const { return selected_; }

  // one camera frame through the device (ope_track_pose)
  Matrix4f localize(const std::vector<Cloud::Ptr> &clusters, double &fitnessScore, double &alignedStrength) {
    selected_ = -1;
    if (clusters.empty()) { branch_ = NO_CLUSTERS; return pose_; }
    if (firstFrame) return first(clusters, fitnessScore, alignedStrength);
    ope_ctx *ctx = compat::default_context();
    const bool skip_coarse = !(poseEstimator.fineFitness() > 0.0001);
    // (ope_track_pose's coarse stage is SAC-IA and its fine stage runs no global rejectors: another coarse method, or an estimator
    // with fine rejectors, takes the loop, one estimateFinalPose at a time)
    if (!ctx || poseEstimator.coarseMethod() != PoseEstimator::COARSE_SAC_IA || poseEstimator.hasFineRejectors() || (skip_coarse && !poseEstimator.alignedSourceIs(*cloudSource)))
      return later_loop(clusters, fitnessScore, alignedStrength);
    if (!model_dev_) model_dev_ = compat::upload(*cloudSourceOriginal, false);
    if (!source_dev_) source_dev_ = compat::upload(*cloudSource, false);
    std::vector<std::shared_ptr<compat::CloudHandle>> held;
    std::vector<const ope_cloud *> hs;
    for (const Cloud::Ptr &c : clusters) { held.push_back(compat::upload(*c, false)); hs.push_back(held.back()->h); }
    ope_track_params p;
    ope_track_default_params(&p);
    p.final.coarse.sacia.seed = poseEstimator.sacIaSeed();
    if (poseEstimator.useSelfOccludedRejector()) { p.final.icp.use_self_occluded_rej = 1; p.final.icp.self_occluded_thr = 0.6; }   // :291
    ope_track_result r;
    std::vector<ope_final_batch_result> re(clusters.size());
    auto aligned = std::make_shared<compat::CloudHandle>();
    if (!model_dev_->h || !source_dev_->h ||
        ope_track_pose(ctx, model_dev_->h, source_dev_->h, poseEstimator.fineFitness(), poseEstimator.coarseCalls(), hs.size(), hs.data(), &p, &r,
                       nullptr, re.data(), &aligned->h) != OPE_OK) {
      compat::log_error("track_pose (running the reference's loop on the host)", ctx);
      return later_loop(clusters, fitnessScore, alignedStrength);
    }
    switch (r.gate.branch) {
      case OPE_TRACK_GATED:
        branch_ = GATED;
        selected_ = r.selected;
        pose_ = poseEstimator.replayTrackedFrame(cloudSource, r, fitnessScore, alignedStrength);
        source_dev_ = aligned;   // the next frame's source, already on the device
        break;
      case OPE_TRACK_REALIGN_ALL:
        branch_ = REALIGN;
        *cloudSource = *cloudSourceOriginal;
        pose_ = poseEstimator.replayCandidates(cloudSource, re, r.selected, fitnessScore, alignedStrength, selected_);
        source_dev_.reset();
        break;
      case OPE_TRACK_REALIGN_LOOP:   // the coarse stages would be skipped: the loop one call at a time
        branch_ = REALIGN;
        realign_loop(clusters, fitnessScore, alignedStrength);
        break;
      default:
        branch_ = NOTHING;
        break;
    }
    return pose_;
  }

  // the same frame by the reference's own loop (rosinterface.cpp:243-313): host centroids, estimateFinalPose one call at a time
  Matrix4f localizeLoop(const std::vector<Cloud::Ptr> &clusters, double &fitnessScore, double &alignedStrength) {
    selected_ = -1;
    if (clusters.empty()) { branch_ = NO_CLUSTERS; return pose_; }
    if (firstFrame) {
      branch_ = FIRST;
      for (size_t i = 0; i < clusters.size(); ++i) {
        *cloudSource = *cloudSourceOriginal;
        if (!clusters[i]->empty()) pose_ = poseEstimator.estimateFinalPose(cloudSource, clusters[i], fitnessScore, alignedStrength);
        if (fitnessScore < 0.0001 || alignedStrength > 0.4) { selected_ = (int)i; break; }
      }
      firstFrame = false;
      return pose_;
    }
    return later_loop(clusters, fitnessScore, alignedStrength);
  }

  // pcl::compute3DCentroid: sequential float sums in the cloud's order; every point of a dense cloud, the finite ones otherwise
  static void centroid(const Cloud &c, bool dense, float out[3]) {
    float s[3] = {0.f, 0.f, 0.f};
    unsigned n = 0;
    for (const auto &q : c.points) {
      if (!dense && !(std::isfinite(q.x) && std::isfinite(q.y) && std::isfinite(q.z))) continue;
      s[0] += q.x; s[1] += q.y; s[2] += q.z;
      ++n;
    }
    for (int d = 0; d < 3; ++d) out[d] = n ? s[d] / (float)n : 0.f;
  }

 private:
  Matrix4f first(const std::vector<Cloud::Ptr> &clusters, double &fitnessScore, double &alignedStrength) {
    branch_ = FIRST;
    *cloudSource = *cloudSourceOriginal;
    pose_ = poseEstimator.estimateFinalPoseCandidates(cloudSource, clusters, fitnessScore, alignedStrength, selected_);
    firstFrame = false;
    source_dev_.reset();
    return pose_;
  }

  // the re-align of the reference's later frame (:304-313): the candidate loop from the original model, one call at a time
  void realign_loop(const std::vector<Cloud::Ptr> &clusters, double &fitnessScore, double &alignedStrength) {
    source_dev_.reset();
    for (size_t i = 0; i < clusters.size(); ++i) {
      *cloudSource = *cloudSourceOriginal;
      if (!clusters[i]->empty()) pose_ = poseEstimator.estimateFinalPose(cloudSource, clusters[i], fitnessScore, alignedStrength);
      if (fitnessScore < 0.0001 || alignedStrength > 0.4) { selected_ = (int)i; break; }
    }
  }

  // rosinterface.cpp:264-313 written out (the cluster clouds are dense: objectsegmentationplane.cpp; cloudSource is not)
  Matrix4f later_loop(const std::vector<Cloud::Ptr> &clusters, double &fitnessScore, double &alignedStrength) {
    source_dev_.reset();
    double distance = 10.0;
    branch_ = NOTHING;
    for (size_t i = 0; i < clusters.size(); ++i) {
      float cc[3], cm[3];
      centroid(*clusters[i], true, cc);
      centroid(*cloudSource, false, cm);
      const float dx = cc[0] - cm[0], dy = cc[1] - cm[1], dz = cc[2] - cm[2];
      distance = (float)std::sqrt((double)((dx * dx + dy * dy) + dz * dz));
      if (distance < 0.05 && !clusters[i]->empty()) {
        pose_ = poseEstimator.estimateFinalPose(cloudSource, clusters[i], fitnessScore, alignedStrength);
        branch_ = GATED;
        selected_ = (int)i;
        return pose_;
      }
    }
    if (distance > 0.05) {
      branch_ = REALIGN;
      realign_loop(clusters, fitnessScore, alignedStrength);
    }
    return pose_;
  }

  PoseEstimator poseEstimator;
  Cloud::Ptr cloudSourceOriginal, cloudSource;
  bool firstFrame = true;
  Matrix4f pose_ = Matrix4f::Identity();
  int branch_ = NO_CLUSTERS, selected_ = -1;
  std::shared_ptr<compat::CloudHandle> model_dev_, source_dev_;
};

}  // namespace ope
