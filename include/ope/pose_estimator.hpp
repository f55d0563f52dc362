// pose_estimator.hpp — the reference's PoseEstimator (DetectAndLocalize/include/poseestimator.h:47-84,
// src/poseestimator.cpp:3-448) on the façade: same public interface, argument meaning, cross-frame state and guard
// behaviour, with every PCL object replaced by its ope::compat counterpart (GPU through the C ABI).
//
//     ope::PoseEstimator poseEstimator;                                   // rosinterface.h:54 holds one per process
//     pose = poseEstimator.estimateFinalPose(cloudSource, cloudTargetSeg, fitnessScore, alignedStrength);   // rosinterface.cpp:250
//
// What the class keeps from the reference, on purpose:
//   * coarse stage only while the previous fine fit scored worse than 1e-4 (poseestimator.cpp:399);
//   * pose = coarsePose * finePose and finalPose = rigidmodelPose * pose, products in the reference's order (quirk Q4);
//   * alignedSource / cloudModel / firstTimePose / fitnessScoreFine / alignedStrength survive between frames;
//   * "< 10 target features" and "< 100 target points" return identity exactly where the reference does;
//   * the caller's source cloud is overwritten with alignedSource (:441), estimateFinePose replaces its argument (:360);
//   * pcl::ScopeTime("Initial Alignment") / ("Final Alignment") around the two align() calls (:61,:349).
// Two knobs PCL does not have: the SAC-IA stream is seeded explicitly (PCL draws from an unseeded rand(); the
// k-th coarse call uses seed + k) and the self-occlusion rejector is opt-in (in the reference it depends on
// the PCL version and on an ODR accident).
#pragma once

#include <cstring>
#include <memory>
#include <vector>

#include "pcl_compat.hpp"

namespace ope {

class PoseEstimator {
 public:
  typedef compat::PointXYZRGB PointT;
  typedef compat::PointCloud<PointT> Cloud;
  typedef compat::PointCloud<compat::Normal> NormalCloud;
  typedef compat::PointCloud<compat::FPFHSignature33> FeatureCloud;
  typedef compat::PointCloud<compat::PointXYZRGBNormal> CloudN;
  typedef compat::Matrix4f Matrix4f;

  PoseEstimator() : alignedSource(new Cloud), cloudModel(new Cloud) {}

  // the coarse aligner: SAC-IA (the reference's live code, the default), the prerejective block the reference keeps commented out, or
  // its other commented block: feature matches, CorrespondenceRejectorSampleConsensus, the SVD over what remains
  enum CoarseMethod { COARSE_SAC_IA = 0, COARSE_PREREJECTIVE = 1, COARSE_CORRESPONDENCES = 2 };
  void setCoarseMethod(CoarseMethod m) { coarse_method_ = m; }
  CoarseMethod coarseMethod() const { return coarse_method_; }
  // estimateFinalPoseCandidates with COARSE_PREREJECTIVE: all clusters in one ope_final_pose_batch_prerejective call instead of one
  // estimateFinalPose at a time (off by default; SAC-IA always batches; COARSE_CORRESPONDENCES ignores this switch and has its own,
  // setCorrespondencesBatch)
  void setCoarseBatch(bool on) { coarse_batch_ = on; }
  bool coarseBatch() const { return coarse_batch_; }
  // that one call makes its draws on the device (ope_prerejective_set_draws, OPE_DRAWS_DEVICE) instead of in a host loop; the poses
  // are the same.  Off by default; takes effect only together with COARSE_PREREJECTIVE and setCoarseBatch(true).  Off, the estimator
  // does not touch the context's mode.
  void setCoarseDeviceDraws(bool on) { coarse_device_draws_ = on; }
  bool coarseDeviceDraws() const { return coarse_device_draws_; }
  // estimateFinalPoseCandidates with COARSE_CORRESPONDENCES: all clusters in one ope_final_pose_batch_correspondences call instead of
  // one estimateFinalPose at a time (off by default)
  void setCorrespondencesBatch(bool on) { correspondences_batch_ = on; }
  bool correspondencesBatch() const { return correspondences_batch_; }
  void setSacIaSeed(uint64_t seed) { sacia_seed_ = seed; }
  void setUseSelfOccludedRejector(bool on) { use_self_occluded_ = on; }
  // The rejectors estimateFinePose's list keeps commented out (:250-292, 3.1 median distance, 3.2 one to one, 3.5 var trimmed), in
  // the order added, behind the surface-normal rejector.  They run inside the single-cluster estimateFinePose.  With rejectors set
  // estimateFinalPoseCandidates and ope::ObjectTracker run the reference's loop, one estimateFinalPose at a time, unless
  // setFineRejectorBatch(true) sends the candidates through ope_final_pose_batch_rejectors (below); the tracked frame takes no list.
  void addFineRejector(const compat::registration::CorrespondenceRejector::Ptr &r) { if (r) fine_rejectors_.push_back(r); }
  void clearFineRejectors() { fine_rejectors_.clear(); }
  bool hasFineRejectors() const { return !fine_rejectors_.empty(); }
  // estimateFinalPoseCandidates with fine rejectors: all clusters in one ope_final_pose_batch_rejectors call (the list applied inside
  // the batched ICP kernel) instead of one estimateFinalPose at a time.  Off by default; needs COARSE_SAC_IA and every fine
  // rejector being one of the three global ones (median distance, one to one, var trimmed), else the loop runs as without it.
  void setFineRejectorBatch(bool on) { fine_rejector_batch_ = on; }
  bool fineRejectorBatch() const { return fine_rejector_batch_; }
  // diagnostics of the last estimateFinalPose call
  Matrix4f lastCoarsePose() const { return last_coarse_; }
  Matrix4f lastFinePose() const { return last_fine_; }
  Matrix4f lastRigidModelPose() const { return last_rigid_; }
  int lastIcpIterations() const { return last_icp_iterations_; }
  int coarseCalls() const { return coarse_calls_; }

  // :131-158  UniformSampling(radius = leafSize) -> the survivors -> NormalEstimation(k = 30) on them
  void subSampleAndCalculateNormals(Cloud::Ptr p_inputCloud, Cloud::Ptr &p_inputCloudSubSampled, NormalCloud::Ptr &p_inputCloudSubSampledNormal,
                                    double leafSize) {
    p_inputCloudSubSampled.reset(new Cloud);
    compat::PointCloud<int> keyPointIndices;
    uniSamp.setInputCloud(p_inputCloud);
    uniSamp.setRadiusSearch(leafSize);
    uniSamp.compute(keyPointIndices);
    compat::copyPointCloud(*p_inputCloud, keyPointIndices.points, *p_inputCloudSubSampled);
    p_inputCloudSubSampledNormal.reset(new NormalCloud);
    normEst.setSearchMethod(std::make_shared<compat::search::KdTree<PointT>>());
    normEst.setKSearch(30);
    normEst.setInputCloud(p_inputCloudSubSampled);
    normEst.compute(*p_inputCloudSubSampledNormal);
  }

  // :110-128  key points at 1 cm REPLACE the input cloud; FPFH with a 3 cm radius on them
  void getFpfhFeatures(Cloud::Ptr &p_inputCloud, FeatureCloud::Ptr &cloudFeatures, Cloud::Ptr &cloudKeyPoints) {
    Cloud::Ptr sub;
    NormalCloud::Ptr nrm;
    subSampleAndCalculateNormals(p_inputCloud, sub, nrm, 0.01);
    *p_inputCloud = *sub;
    cloudKeyPoints = sub;
    cloudFeatures.reset(new FeatureCloud);
    fpfhEstimation.setInputCloud(sub);
    fpfhEstimation.setRadiusSearch(0.03);
    fpfhEstimation.setInputNormals(nrm);
    fpfhEstimation.compute(*cloudFeatures);
  }

  // :16-73
  Matrix4f estimateCoarsePose(Cloud::Ptr p_sourceCloud, Cloud::Ptr p_targetCloud) {
    Cloud::Ptr src(new Cloud(*p_sourceCloud)), tgt(new Cloud(*p_targetCloud)), srcKeys, tgtKeys;
    FeatureCloud::Ptr srcFeat, tgtFeat;
    getFpfhFeatures(src, srcFeat, srcKeys);
    getFpfhFeatures(tgt, tgtFeat, tgtKeys);
    if (tgtFeat->points.size() < 10) {   // :40-45
      *alignedSource = *p_sourceCloud;
      std::printf("NO target cloud in Initial Alignment\n");
      return Matrix4f::Identity();
    }
    if (coarse_method_ == COARSE_PREREJECTIVE) return prerejectiveCoarsePose(p_sourceCloud, src, tgt, srcFeat, tgtFeat);
    if (coarse_method_ == COARSE_CORRESPONDENCES) return correspondencesCoarsePose(p_sourceCloud, src, tgt, srcFeat, tgtFeat);
    compat::SampleConsensusInitialAlignment<PointT, PointT, compat::FPFHSignature33> sacia;
    sacia.setInputSource(src);
    sacia.setInputTarget(tgt);
    sacia.setSourceFeatures(srcFeat);
    sacia.setTargetFeatures(tgtFeat);
    sacia.setMaximumIterations(400);          // :55
    sacia.setNumberOfSamples(5);              // :56
    sacia.setCorrespondenceRandomness(5);     // :57
    sacia.setMaxCorrespondenceDistance(0.05); // :58
    sacia.setMinSampleDistance(0.01f);        // :59
    sacia.setSeed(sacia_seed_ + (uint64_t)coarse_calls_++);
    Cloud result;
    {
      compat::ScopeTime t("Initial Alignment");
      sacia.align(result);
    }
    const Matrix4f pose = sacia.getFinalTransformation();
    compat::transformPointCloud(*p_sourceCloud, *alignedSource, pose);   // :66-70, full resolution
    return pose;
  }

  // :161-379
  Matrix4f estimateFinePose(Cloud::Ptr &p_sourceCloud, Cloud::Ptr p_targetCloud) {
    Cloud::Ptr src(new Cloud), tgt(new Cloud);
    std::vector<int> index;
    compat::removeNaNFromPointCloud(*p_sourceCloud, *src, index);   // :186-194
    compat::removeNaNFromPointCloud(*p_targetCloud, *tgt, index);
    CloudN::Ptr srcPN = withNormals(src), tgtPN = withNormals(tgt);  // :196-216, sub-sampling at 8 mm
    if (tgtPN->points.size() < 100) {   // :218-223
      std::printf("NO target cloud in Final Alignment\n");
      return Matrix4f::Identity();
    }
    typedef compat::registration::CorrespondenceEstimationNormalShooting<compat::PointXYZRGBNormal, compat::PointXYZRGBNormal, compat::PointXYZRGBNormal> NS;
    NS::Ptr corrEstNormShoot(new NS);
    corrEstNormShoot->setInputSource(srcPN);
    corrEstNormShoot->setSourceNormals(srcPN);
    corrEstNormShoot->setInputTarget(tgtPN);
    corrEstNormShoot->setKSearch(20);   // :246
    compat::registration::CorrespondenceRejectorSurfaceNormal::Ptr corrRejSurNorm(new compat::registration::CorrespondenceRejectorSurfaceNormal);
    corrRejSurNorm->initializeDataContainer<compat::PointXYZRGBNormal, compat::PointXYZRGBNormal>();
    corrRejSurNorm->setThreshold(0.7);  // :272
    compat::registration::CorrespondenceRejectorSelfOccludedNormal::Ptr corrRejSelfNorm(new compat::registration::CorrespondenceRejectorSelfOccludedNormal);
    corrRejSelfNorm->setThreshold(0.6); // :291
    compat::registration::TransformationEstimationSVD<compat::PointXYZRGBNormal, compat::PointXYZRGBNormal>::Ptr transfEstSvd(
        new compat::registration::TransformationEstimationSVD<compat::PointXYZRGBNormal, compat::PointXYZRGBNormal>);
    compat::IterativeClosestPointWithNormals<compat::PointXYZRGBNormal, compat::PointXYZRGBNormal> icp;
    icp.setInputSource(srcPN);
    icp.setInputTarget(tgtPN);
    icp.setMaximumIterations(100);         // :322
    icp.setTransformationEpsilon(1e-8);    // :325
    icp.setEuclideanFitnessEpsilon(1e-8);  // :328
    icp.setCorrespondenceEstimation(corrEstNormShoot);
    icp.addCorrespondenceRejector(corrRejSurNorm);
    if (use_self_occluded_) icp.addCorrespondenceRejector(corrRejSelfNorm);
    for (const auto &r : fine_rejectors_) icp.addCorrespondenceRejector(r);
    icp.setTransformationEstimation(transfEstSvd);
    CloudN cloudAligned;
    {
      compat::ScopeTime t("Final Alignment");
      icp.align(cloudAligned);
    }
    fitnessScoreFine = icp.getFitnessScore();   // :354
    const Matrix4f pose = icp.getFinalTransformation();
    Cloud::Ptr moved(new Cloud);
    compat::transformPointCloud(*p_sourceCloud, *moved, pose);   // :358-360
    *p_sourceCloud = *moved;
    alignedStrength = icp.getAlignStrength();   // :363
    last_icp_iterations_ = icp.getNumberOfIterations();
    std::printf("Aligned Strength : %g\n", alignedStrength);
    return pose;
  }

  // :383-448
  Matrix4f estimateFinalPose(Cloud::Ptr &p_sourceCloud, Cloud::Ptr p_targetCloud, double &fitnessScore, double &alignStrength) {
    if (firstTimePose == 0) *cloudModel = *p_sourceCloud;   // the original model, kept for the re-anchoring fit
    ++firstTimePose;
    const bool have_target = !p_targetCloud->empty();
    Matrix4f coarsePose = Matrix4f::Identity(), finePose = Matrix4f::Identity();
    if (have_target && fitnessScoreFine > 0.0001) coarsePose = estimateCoarsePose(p_sourceCloud, p_targetCloud);
    if (have_target) finePose = estimateFinePose(alignedSource, p_targetCloud);
    finish(p_sourceCloud, coarsePose, finePose);
    fitnessScore = fitnessScoreFine;
    alignStrength = alignedStrength;
    return finalPose;
  }

  // The reference's first-frame candidate loop (rosinterface.cpp:243-262) in one call:
  //     for each cluster: source = a copy of the original model; if the cluster is not empty, estimateFinalPose(source, cluster);
  //                       stop once fitness < 1e-4 or strength > 0.4
  // p_sourceCloud is the original model on entry.  Runs ope_final_pose_batch (with COARSE_PREREJECTIVE and setCoarseBatch(true):
  // ope_final_pose_batch_prerejective; with COARSE_CORRESPONDENCES and setCorrespondencesBatch(true): ope_final_pose_batch_correspondences;
  // without their switches those methods run the loop as written above) over all clusters, then leaves the estimator and
  // p_sourceCloud exactly as that loop would: coarse calls counted only for clusters that reached SAC-IA, fitnessScoreFine /
  // alignedStrength from the last cluster (up to the selected one) that ran a fine ICP, alignedSource / cloudModel / firstTimePose
  // / the last* diagnostics as after the last non-empty cluster it processed; p_sourceCloud holds alignedSource, or the original
  // model if the last cluster it visited was empty.  selected = the accepted cluster or -1; the pose is that of the last
  // estimateFinalPose the loop made (finalPose unchanged if every cluster is empty).  When fitnessScoreFine <= 1e-4 on entry
  // (the coarse stage would be skipped) or the batch refuses the clouds (ope.h: OPE_COARSE_MAX_POINTS / _MAX_KEYS), the loop runs
  // as written above, one estimateFinalPose at a time.
  Matrix4f estimateFinalPoseCandidates(Cloud::Ptr &p_sourceCloud, const std::vector<Cloud::Ptr> &clusters, double &fitnessScore,
                                       double &alignStrength, int &selected) {
    selected = -1;
    const Cloud original(*p_sourceCloud);
    std::vector<ope_final_batch_result> res(clusters.size());
    int32_t sel = -1;
    // (ope_final_pose_batch's coarse stage is SAC-IA; the prerejective batch is opt-in: setCoarseBatch)
    // (with fine rejectors the batch is opt-in too, SAC-IA only, and every rejector must be a global one: setFineRejectorBatch)
    std::vector<ope_global_rejector> glist;
    bool list_ok = fine_rejectors_.empty();
    if (!list_ok && fine_rejector_batch_ && coarse_method_ == COARSE_SAC_IA && fine_rejectors_.size() <= (size_t)OPE_GREJ_MAX) {
      list_ok = true;
      for (const auto &r : fine_rejectors_) {
        ope_global_rejector g;
        if (r->global(g)) glist.push_back(g);
        else list_ok = false;
      }
    }
    bool batched = fitnessScoreFine > 0.0001 && !clusters.empty() && list_ok &&
                   (coarse_method_ == COARSE_SAC_IA || (coarse_method_ == COARSE_PREREJECTIVE && coarse_batch_) ||
                    (coarse_method_ == COARSE_CORRESPONDENCES && correspondences_batch_));
    if (batched) {
      ope_ctx *ctx = compat::default_context();
      auto model = compat::upload(original, false);
      std::vector<std::shared_ptr<compat::CloudHandle>> held;
      std::vector<const ope_cloud *> hs;
      for (const Cloud::Ptr &c : clusters) { held.push_back(compat::upload(*c, false)); hs.push_back(held.back()->h); }
      ope_final_params p;
      ope_final_default_params(&p);
      p.coarse.sacia.seed = sacia_seed_ + (uint64_t)coarse_calls_;   // the k-th SAC-IA call draws with seed + k
      if (use_self_occluded_) { p.icp.use_self_occluded_rej = 1; p.icp.self_occluded_thr = 0.6; }   // :291
      if (coarse_method_ == COARSE_PREREJECTIVE) {
        ope_prerejective_params q;
        ope_prerejective_default_params(&q);
        q.max_iterations = 50000;          // the literals of prerejectiveCoarsePose (:97-102)
        q.nr_samples = 3;
        q.k_correspondences = 5;
        q.similarity_threshold = 0.8f;
        q.max_corr_dist = 0.15;
        q.inlier_fraction = 0.25f;
        q.seed = sacia_seed_ + (uint64_t)coarse_calls_;   // the k-th coarse call draws with seed + k
        // (the context is shared: with the switch on, the mode it had comes back after the call; with the switch off the context
        // is left alone, so a mode set directly with ope_prerejective_set_draws holds)
        int draws_before = OPE_DRAWS_HOST;
        const bool set_draws = ctx && coarse_device_draws_;
        if (set_draws) { ope_prerejective_get_draws(ctx, &draws_before); ope_prerejective_set_draws(ctx, OPE_DRAWS_DEVICE); }
        batched = ctx && model->h &&
                  ope_final_pose_batch_prerejective(ctx, model->h, hs.size(), hs.data(), &p, &q, nullptr, res.data(), &sel) == OPE_OK;
        if (set_draws) ope_prerejective_set_draws(ctx, draws_before);
      } else if (coarse_method_ == COARSE_CORRESPONDENCES) {
        ope_corr_sac_params q;
        ope_corr_sac_default_params(&q);   // (PCL's fixed seed: every rejector of the loop is a fresh object)
        q.max_iterations = 10000;          // the literals of correspondencesCoarsePose (:55-56)
        q.inlier_threshold = 0.08;
        batched = ctx && model->h &&
                  ope_final_pose_batch_correspondences(ctx, model->h, hs.size(), hs.data(), &p, &q, nullptr, res.data(), &sel) == OPE_OK;
      } else if (!glist.empty()) {
        batched = ctx && model->h &&
                  ope_final_pose_batch_rejectors(ctx, model->h, hs.size(), hs.data(), &p, glist.data(), glist.size(), nullptr, res.data(), &sel) == OPE_OK;
      } else {
        batched = ctx && model->h && ope_final_pose_batch(ctx, model->h, hs.size(), hs.data(), &p, nullptr, res.data(), &sel) == OPE_OK;
      }
      if (!batched && ctx) compat::log_error("final_pose_batch (running the loop one cluster at a time)", ctx);
    }
    if (!batched) {
      Matrix4f pose = finalPose;
      for (size_t i = 0; i < clusters.size(); ++i) {
        *p_sourceCloud = original;
        if (clusters[i]->empty()) continue;
        pose = estimateFinalPose(p_sourceCloud, clusters[i], fitnessScore, alignStrength);
        if (fitnessScore < 0.0001 || alignStrength > 0.4) { selected = (int)i; break; }
      }
      fitnessScore = fitnessScoreFine;
      alignStrength = alignedStrength;
      return pose;
    }
    return replayCandidates(p_sourceCloud, res, sel, fitnessScore, alignStrength, selected);
  }

  // ---- the narrow state hand-over of ope::ObjectTracker (object_tracker.hpp): what ope_track_pose needs on entry, and the
  // replay of its results into this estimator exactly as the calls it stands for would have left it
  double fineFitness() const { return fitnessScoreFine; }
  uint64_t sacIaSeed() const { return sacia_seed_; }
  bool useSelfOccludedRejector() const { return use_self_occluded_; }
  // the coarse-skipped fine stage starts from alignedSource (:404): the tracker's device source must be that cloud
  bool alignedSourceIs(const Cloud &c) const {
    return c.size() == alignedSource->size() && (c.empty() || !std::memcmp(c.points.data(), alignedSource->points.data(), sizeof(PointT) * c.size()));
  }
  // estimateFinalPoseCandidates' batch, from its results: p_sourceCloud = the original model on entry
  Matrix4f replayCandidates(Cloud::Ptr &p_sourceCloud, const std::vector<ope_final_batch_result> &res, int32_t sel, double &fitnessScore,
                            double &alignStrength, int &selected) {
    const Cloud original(*p_sourceCloud);
    const size_t last = sel >= 0 ? (size_t)sel : res.size() - 1;   // the last cluster the loop visits
    int applied = -1;
    for (size_t i = 0; i <= last; ++i) {
      const ope_final_batch_result &r = res[i];
      if (r.status == OPE_FINAL_EMPTY_TARGET) continue;
      if (firstTimePose == 0) *cloudModel = original;
      ++firstTimePose;
      if (r.coarse.status == OPE_COARSE_OK) ++coarse_calls_;
      if (r.status == OPE_FINAL_OK || r.status == OPE_FINAL_FEW_TARGET_FEATURES) {
        fitnessScoreFine = r.fine.fitness;
        alignedStrength = r.fine.result.align_strength;
        last_icp_iterations_ = r.fine.result.iterations;
      }
      applied = (int)i;
    }
    if (applied >= 0) {
      const ope_final_batch_result &r = res[(size_t)applied];
      Matrix4f coarsePose = Matrix4f::Identity(), finePose = Matrix4f::Identity();
      std::memcpy(coarsePose.m, r.coarse.T, sizeof coarsePose.m);
      if (r.coarse.status == OPE_COARSE_OK) compat::transformPointCloud(original, *alignedSource, coarsePose);   // :66-70
      else *alignedSource = original;                                                                            // :40-45
      if (r.status != OPE_FINAL_FEW_FINE_POINTS) {   // :358-360
        std::memcpy(finePose.m, r.fine.T, sizeof finePose.m);
        Cloud::Ptr moved(new Cloud);
        compat::transformPointCloud(*alignedSource, *moved, finePose);
        *alignedSource = *moved;
      }
      *p_sourceCloud = original;
      finish(p_sourceCloud, coarsePose, finePose);
    }
    if (res[last].status == OPE_FINAL_EMPTY_TARGET) *p_sourceCloud = original;   // the loop's copy before an empty cluster
    selected = sel;
    fitnessScore = fitnessScoreFine;
    alignStrength = alignedStrength;
    return finalPose;
  }
  // estimateFinalPose(p_sourceCloud, cluster) from ope_track_pose's GATED result (the rigid fit came from the device)
  Matrix4f replayTrackedFrame(Cloud::Ptr &p_sourceCloud, const ope_track_result &r, double &fitnessScore, double &alignStrength) {
    if (firstTimePose == 0) *cloudModel = *p_sourceCloud;
    ++firstTimePose;
    Matrix4f coarsePose = Matrix4f::Identity(), finePose = Matrix4f::Identity(), rigid = Matrix4f::Identity();
    if (r.coarse_status != OPE_TRACK_COARSE_SKIPPED) {
      std::memcpy(coarsePose.m, r.coarse, sizeof coarsePose.m);
      if (r.coarse_status == OPE_COARSE_OK) {
        ++coarse_calls_;
        compat::transformPointCloud(*p_sourceCloud, *alignedSource, coarsePose);   // :66-70
      } else {
        *alignedSource = *p_sourceCloud;                                           // :40-45
      }
    }
    if (r.status != OPE_FINAL_FEW_FINE_POINTS) {   // :354-363
      std::memcpy(finePose.m, r.fine, sizeof finePose.m);
      Cloud::Ptr moved(new Cloud);
      compat::transformPointCloud(*alignedSource, *moved, finePose);
      *alignedSource = *moved;
      fitnessScoreFine = r.fitness;
      alignedStrength = r.icp.align_strength;
      last_icp_iterations_ = r.icp.iterations;
    }
    std::memcpy(rigid.m, r.rigid, sizeof rigid.m);
    finalPose = rigid * (coarsePose * finePose);   // :421, :439
    *p_sourceCloud = *alignedSource;               // :441
    last_coarse_ = coarsePose; last_fine_ = finePose; last_rigid_ = rigid;
    fitnessScore = fitnessScoreFine;
    alignStrength = alignedStrength;
    return finalPose;
  }

 private:
  // BuildModel/src/poseestimator.cpp:92-107, the block the reference keeps commented out, in SAC-IA's place: the same key points and
  // features, the k-th coarse call draws with seed + k; without a converged alignment the pose is the identity
  Matrix4f prerejectiveCoarsePose(const Cloud::Ptr &p_sourceCloud, const Cloud::Ptr &src, const Cloud::Ptr &tgt, const FeatureCloud::Ptr &srcFeat,
                                  const FeatureCloud::Ptr &tgtFeat) {
    compat::SampleConsensusPrerejective<PointT, PointT, compat::FPFHSignature33> sacPreRej;
    sacPreRej.setInputSource(src);
    sacPreRej.setSourceFeatures(srcFeat);
    sacPreRej.setInputTarget(tgt);
    sacPreRej.setTargetFeatures(tgtFeat);
    sacPreRej.setMaximumIterations(50000);          // :97
    sacPreRej.setNumberOfSamples(3);                // :98
    sacPreRej.setCorrespondenceRandomness(5);       // :99
    sacPreRej.setSimilarityThreshold(0.8f);         // :100
    sacPreRej.setMaxCorrespondenceDistance(0.15);   // :101
    sacPreRej.setInlierFraction(0.25f);             // :102
    sacPreRej.setSeed(sacia_seed_ + (uint64_t)coarse_calls_++);
    Cloud result;
    {
      compat::ScopeTime t("Initial Alignment");
      sacPreRej.align(result);
    }
    const Matrix4f pose = sacPreRej.hasConverged() ? sacPreRej.getFinalTransformation() : Matrix4f::Identity();
    compat::transformPointCloud(*p_sourceCloud, *alignedSource, pose);
    return pose;
  }

  // BuildModel/src/poseestimator.cpp:43-60 and :111-113, the other block the reference keeps commented out, in SAC-IA's place: the
  // same key points and features; FPFH matches, the rejector with its 10 000 iterations and 0.08, the SVD over the remaining matches
  // (over all of them when RANSAC finds no model, as those lines would).  The draws start from PCL's fixed seed: no call counter
  // enters them, but the call is counted like the other aligners'.
  Matrix4f correspondencesCoarsePose(const Cloud::Ptr &p_sourceCloud, const Cloud::Ptr &src, const Cloud::Ptr &tgt, const FeatureCloud::Ptr &srcFeat,
                                     const FeatureCloud::Ptr &tgtFeat) {
    ++coarse_calls_;
    Matrix4f pose = Matrix4f::Identity();
    {
      compat::ScopeTime t("Initial Alignment");
      std::shared_ptr<compat::Correspondences> correspondences(new compat::Correspondences);
      compat::registration::CorrespondenceEstimation<compat::FPFHSignature33, compat::FPFHSignature33> cest;   // :43-47
      cest.setInputSource(srcFeat);
      cest.setInputTarget(tgtFeat);
      cest.determineCorrespondences(*correspondences);
      compat::registration::CorrespondenceRejectorSampleConsensus<PointT> rejector;                             // :49-60
      rejector.setInputSource(src);
      rejector.setInputTarget(tgt);
      rejector.setInputCorrespondences(correspondences);
      rejector.setMaximumIterations(10000);   // :55
      rejector.setInlierThreshold(0.08);      // :56
      compat::Correspondences remaining;
      rejector.getCorrespondences(remaining);
      compat::registration::TransformationEstimationSVD<PointT, PointT> transEst;                               // :111-113
      transEst.estimateRigidTransformation(*src, *tgt, remaining, pose);
    }
    compat::transformPointCloud(*p_sourceCloud, *alignedSource, pose);
    return pose;
  }

  // sub-sample at 8 mm, normals (k = 30), xyz + normal packed into PointXYZRGBNormal, NaN normals dropped (:196-216)
  CloudN::Ptr withNormals(const Cloud::Ptr &cloud) {
    Cloud::Ptr sub;
    NormalCloud::Ptr nrm;
    subSampleAndCalculateNormals(cloud, sub, nrm, 0.008);
    CloudN::Ptr out(new CloudN);
    for (size_t i = 0; i < sub->size() && i < nrm->size(); ++i) {
      const compat::Normal &n = (*nrm)[i];
      if (!std::isfinite(n.normal_x) || !std::isfinite(n.normal_y) || !std::isfinite(n.normal_z)) continue;
      compat::PointXYZRGBNormal q;
      q.x = (*sub)[i].x; q.y = (*sub)[i].y; q.z = (*sub)[i].z; q.rgb = (*sub)[i].rgb;
      q.normal_x = n.normal_x; q.normal_y = n.normal_y; q.normal_z = n.normal_z; q.curvature = n.curvature;
      out->push_back(q);
    }
    return out;
  }

  // the end of estimateFinalPose (:421-441): pose = coarse * fine, the re-anchoring fit of the incoming source against the stored
  // model (SVD over identity correspondences, :425-436), finalPose = rigidmodelPose * pose, the source replaced by alignedSource
  void finish(Cloud::Ptr &p_sourceCloud, const Matrix4f &coarsePose, const Matrix4f &finePose) {
    const Matrix4f pose = coarsePose * finePose;   // :421
    Matrix4f rigidmodelPose = Matrix4f::Identity();
    {
      compat::Correspondences corres(cloudModel->points.size());
      for (size_t i = 0; i < corres.size(); ++i) corres[i].index_query = corres[i].index_match = (int)i;
      if (!corres.empty() && p_sourceCloud->size() >= corres.size()) svd.estimateRigidTransformation(*cloudModel, *p_sourceCloud, corres, rigidmodelPose);
    }
    finalPose = rigidmodelPose * pose;   // :439
    *p_sourceCloud = *alignedSource;     // :441
    last_coarse_ = coarsePose; last_fine_ = finePose; last_rigid_ = rigidmodelPose;
  }

  // state that crosses frames (poseestimator.h:50-53)
  Cloud::Ptr alignedSource, cloudModel;
  double fitnessScoreFine = 10.0, alignedStrength = 0.0;   // "random high value" (:6)
  Matrix4f finalPose = Matrix4f::Identity();
  int firstTimePose = 0;
  // objects (poseestimator.h:56-60)
  compat::FPFHEstimation<PointT, compat::Normal, compat::FPFHSignature33> fpfhEstimation;
  compat::UniformSampling<PointT> uniSamp;
  compat::NormalEstimation<PointT, compat::Normal> normEst;
  compat::registration::TransformationEstimationSVD<PointT, PointT> svd;
  // knobs and diagnostics
  uint64_t sacia_seed_ = 1;
  CoarseMethod coarse_method_ = COARSE_SAC_IA;
  int coarse_calls_ = 0;
  bool coarse_batch_ = false, correspondences_batch_ = false, fine_rejector_batch_ = false, coarse_device_draws_ = false;
  bool use_self_occluded_ = false;
  std::vector<compat::registration::CorrespondenceRejector::Ptr> fine_rejectors_;   // addFineRejector, in the order added
  Matrix4f last_coarse_ = Matrix4f::Identity(), last_fine_ = Matrix4f::Identity(), last_rigid_ = Matrix4f::Identity();
  int last_icp_iterations_ = 0;
};

}  // namespace ope
