// detect_and_localize.cpp — config C1 from files: what DetectAndLocalize does per frame once a table-top cluster has
// been cut out (rosinterface.cpp:80 loads the model .pcd, :250 calls PoseEstimator::estimateFinalPose(model, cluster)),
// with pcl:: replaced by the façade and the GPU library behind it.
//
//   detect_and_localize <model.pcd> <scene.pcd> [<scene2.pcd> ...] [--seed N] [--self-occluded] [--candidates | --candidates-loop]
//
// One line per frame on stdout, parsed by tests/test_gpu_detect_and_localize.py:
//   frame <k> fitness <f> strength <s> coarse_calls <n> icp_iterations <n> final <16 floats, column-major> coarse <16> fine <16> rigid <16>
// and `aligned <path>` after saving the aligned model of the last frame next to the first scene file.
// --candidates: the scene files are the clusters of ONE first frame (rosinterface.cpp:243-262), checked by
// PoseEstimator::estimateFinalPoseCandidates in one call; --candidates-loop: the same frame by the reference's loop of
// estimateFinalPose.  Either prints `candidates selected <i> clusters <n>`, then one `frame 1 ...` line.
//
//   detect_and_localize --segment <model.pcd> <not_plane.pcd> [--seed N] [--self-occluded]
// The first frame from the non-plane cloud: ObjectSegmentationPlane::getClusters as the reference writes it
// (pcl::EuclideanClusterExtraction, tolerance 0.05, 300 .. 1e5 points), each cluster copied by index (rosinterface.cpp:246-255),
// then the clusters as --candidates takes them.  Prints `segment clusters <n> sizes <s0> <s1> ...`, then the --candidates lines.
//
//   detect_and_localize --frame <model.pcd> <frame.pcd> [--limits x0 x1 y0 y1 z0 z1] [--seed N] [--self-occluded]
// The first frame from the camera frame itself (rosinterface.cpp:212-262): ProcessingPcd::getPassThrough (three pcl::PassThrough,
// the -l limits; without --limits only non-finite points go), ope::ObjectSegmentationPlane::getSegmentedObjectsOnPlane (plane
// fit, prism, second fit and clusters on the device), then the clusters as --candidates takes them.  Prints
// `segment plane <n>`, `segment clusters <n> sizes <s0> <s1> ...`, then the --candidates lines.
//
//   detect_and_localize --track <model.pcd> --frame <a.pcd> [<b.pcd> ...] [--frame ...] [--seed N] [--self-occluded] [--time]
//   detect_and_localize --track-loop <model.pcd> --frame ... (same)
// DetectAndLocalize's per-frame policy (rosinterface.cpp:226-313) over a sequence of camera frames, one --frame per frame with
// that frame's clusters (none: an empty frame).  --track: ope::ObjectTracker::localize (the gate and the gated pose on the
// device); --track-loop: ObjectTracker::localizeLoop (host compute3DCentroid and estimateFinalPose, as the reference writes it).
// Per frame: `track frame <k> branch <b> selected <i> clusters <n>`, then the `frame ...` line; --time adds `time frame <k> ms <t>`
// (host clock around the synchronised call).
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <chrono>

#include "object_segmentation_plane.hpp"
#include "object_tracker.hpp"
#include "pcd_io.hpp"
#include "pose_estimator.hpp"

namespace pcl = ope::compat;

static void print16(const char *tag, const pcl::Matrix4f &m) {
  std::printf(" %s", tag);
  for (int i = 0; i < 16; ++i) std::printf(" %.9g", (double)m.m[i]);
}

static const char *branch_name(int b) {
  switch (b) {
    case ope::ObjectTracker::FIRST: return "FIRST";
    case ope::ObjectTracker::GATED: return "GATED";
    case ope::ObjectTracker::REALIGN: return "REALIGN";
    case ope::ObjectTracker::NOTHING: return "NOTHING";
    default: return "NO_CLUSTERS";
  }
}

// --track / --track-loop
static int track_main(int argc, char **argv) {
  int mode = 0;   // 1: --track, 2: --track-loop
  std::string model_path;
  std::vector<std::vector<std::string>> frames;
  uint64_t seed = 1;
  bool self_occluded = false, timed = false;
  for (int i = 1; i < argc; ++i) {
    if ((!std::strcmp(argv[i], "--track") || !std::strcmp(argv[i], "--track-loop")) && i + 1 < argc) {
      mode = !std::strcmp(argv[i], "--track") ? 1 : 2;
      model_path = argv[++i];
    } else if (!std::strcmp(argv[i], "--frame")) frames.emplace_back();
    else if (!std::strcmp(argv[i], "--seed") && i + 1 < argc) seed = std::strtoull(argv[++i], nullptr, 10);
    else if (!std::strcmp(argv[i], "--self-occluded")) self_occluded = true;
    else if (!std::strcmp(argv[i], "--time")) timed = true;
    else if (!frames.empty()) frames.back().push_back(argv[i]);
    else { std::fprintf(stderr, "unexpected argument %s\n", argv[i]); return 2; }
  }
  if (!mode || frames.empty()) { std::fprintf(stderr, "usage: %s --track|--track-loop <model.pcd> --frame <cluster.pcd> ... [--frame ...]\n", argv[0]); return 2; }
  typedef ope::PoseEstimator::PointT PointT;
  pcl::PointCloud<PointT> model;
  if (pcl::io::loadPCDFile(model_path, model) != 0) return 3;
  ope::ObjectTracker tracker(model);
  tracker.estimator().setSacIaSeed(seed);
  tracker.estimator().setUseSelfOccludedRejector(self_occluded);
  double fitnessScore = 10.0, alignedStrength = 0.0;   // rosinterface.h: kept across frames
  for (size_t k = 0; k < frames.size(); ++k) {
    std::vector<pcl::PointCloud<PointT>::Ptr> clusters;
    for (const std::string &f : frames[k]) {
      clusters.emplace_back(new pcl::PointCloud<PointT>);
      if (pcl::io::loadPCDFile(f, *clusters.back()) != 0) return 3;
    }
    ope_ctx *ctx = pcl::default_context();
    if (ctx) ope_ctx_sync(ctx);
    const auto t0 = std::chrono::steady_clock::now();
    const pcl::Matrix4f pose = mode == 1 ? tracker.localize(clusters, fitnessScore, alignedStrength)
                                         : tracker.localizeLoop(clusters, fitnessScore, alignedStrength);
    if (ctx) ope_ctx_sync(ctx);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const ope::PoseEstimator &e = tracker.estimator();
    std::printf("track frame %zu branch %s selected %d clusters %zu\n", k + 1, branch_name(tracker.lastBranch()), tracker.lastSelected(),
                clusters.size());
    if (timed) std::printf("time frame %zu ms %.4f\n", k + 1, ms);
    std::printf("frame %zu fitness %.12g strength %.12g coarse_calls %d icp_iterations %d", k + 1, fitnessScore, alignedStrength,
                e.coarseCalls(), e.lastIcpIterations());
    print16("final", pose);
    print16("coarse", e.lastCoarsePose());
    print16("fine", e.lastFinePose());
    print16("rigid", e.lastRigidModelPose());
    std::printf("\n");
  }
  const std::string out = model_path + ".tracked.pcd";
  if (pcl::io::savePCDFile(out, tracker.source(), true) != 0) return 4;
  std::printf("aligned %s\n", out.c_str());
  return 0;
}

int main(int argc, char **argv) {
  for (int i = 1; i < argc; ++i)
    if (!std::strcmp(argv[i], "--track") || !std::strcmp(argv[i], "--track-loop")) return track_main(argc, argv);
  std::vector<std::string> files;
  uint64_t seed = 1;
  bool self_occluded = false;
  int candidates = 0;   // 1: estimateFinalPoseCandidates, 2: the reference's loop
  bool segment = false; // --segment: the clusters come from getClusters over the one scene file (the non-plane cloud)
  bool frame = false;   // --frame: the clusters come from getSegmentedObjectsOnPlane over the one scene file (a camera frame)
  float limits[6] = {-FLT_MAX, FLT_MAX, -FLT_MAX, FLT_MAX, -FLT_MAX, FLT_MAX};
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--seed") && i + 1 < argc) seed = std::strtoull(argv[++i], nullptr, 10);
    else if (!std::strcmp(argv[i], "--self-occluded")) self_occluded = true;
    else if (!std::strcmp(argv[i], "--candidates")) candidates = 1;
    else if (!std::strcmp(argv[i], "--candidates-loop")) candidates = 2;
    else if (!std::strcmp(argv[i], "--segment")) { segment = true; candidates = 1; }
    else if (!std::strcmp(argv[i], "--frame")) { frame = true; candidates = 1; }
    else if (!std::strcmp(argv[i], "--limits") && i + 6 < argc) { for (int d = 0; d < 6; ++d) limits[d] = std::strtof(argv[++i], nullptr); }
    else files.push_back(argv[i]);
  }
  if (files.size() < 2) { std::fprintf(stderr, "usage: %s <model.pcd> <scene.pcd> [more scenes] [--seed N] [--self-occluded] [--candidates | --candidates-loop | --segment | --frame]\n", argv[0]); return 2; }
  typedef ope::PoseEstimator::PointT PointT;
  pcl::PointCloud<PointT>::Ptr cloudSourceOriginal(new pcl::PointCloud<PointT>), cloudSource(new pcl::PointCloud<PointT>);
  if (pcl::io::loadPCDFile(files[0], *cloudSourceOriginal) != 0) return 3;   // rosinterface.cpp:80
  *cloudSource = *cloudSourceOriginal;
  ope::PoseEstimator poseEstimator;
  poseEstimator.setSacIaSeed(seed);
  poseEstimator.setUseSelfOccludedRejector(self_occluded);
  auto print_frame = [&](size_t k, const pcl::Matrix4f &pose, double fitnessScore, double alignedStrength) {
    std::printf("frame %zu fitness %.12g strength %.12g coarse_calls %d icp_iterations %d", k, fitnessScore, alignedStrength,
                poseEstimator.coarseCalls(), poseEstimator.lastIcpIterations());
    print16("final", pose);
    print16("coarse", poseEstimator.lastCoarsePose());
    print16("fine", poseEstimator.lastFinePose());
    print16("rigid", poseEstimator.lastRigidModelPose());
    std::printf("\n");
  };
  if (candidates) {
    std::vector<pcl::PointCloud<PointT>::Ptr> clusters;
    if (segment) {
      // ObjectSegmentationPlane::getClusters as the reference writes it (objectsegmentationplane.cpp:79-93), then each cluster's
      // points copied by index (rosinterface.cpp:246-255)
      pcl::PointCloud<PointT>::Ptr notPlane(new pcl::PointCloud<PointT>);
      if (files.size() != 2 || pcl::io::loadPCDFile(files[1], *notPlane) != 0) return 3;
      pcl::search::KdTree<PointT>::Ptr tree(new pcl::search::KdTree<PointT>);
      std::vector<pcl::PointIndices> cluster_indices;
      pcl::EuclideanClusterExtraction<PointT> ec;
      ec.setClusterTolerance(0.05);
      ec.setMinClusterSize(300);
      ec.setMaxClusterSize(1e5);
      ec.setSearchMethod(tree);
      ec.setInputCloud(notPlane);
      ec.extract(cluster_indices);
      std::printf("segment clusters %zu sizes", cluster_indices.size());
      for (const pcl::PointIndices &it : cluster_indices) {
        pcl::PointCloud<PointT>::Ptr cloudCluster(new pcl::PointCloud<PointT>);
        for (int pit : it.indices) cloudCluster->points.push_back(notPlane->points[pit]);
        cloudCluster->width = (uint32_t)cloudCluster->points.size();
        cloudCluster->height = 1;
        cloudCluster->is_dense = true;
        clusters.push_back(cloudCluster);
        std::printf(" %zu", it.indices.size());
      }
      std::printf("\n");
    }
    if (frame) {
      // rosinterface.cpp:212-213: the pass-through crop, then the table-top segmentation
      pcl::PointCloud<PointT>::Ptr cloudTarget(new pcl::PointCloud<PointT>), cloudPlane;
      if (segment || files.size() != 2 || pcl::io::loadPCDFile(files[1], *cloudTarget) != 0) return 3;
      const char *fields[3] = {"x", "y", "z"};
      for (int d = 0; d < 3; ++d) {   // ProcessingPcd::getPassThrough (processingpcd.cpp:13-33)
        pcl::PointCloud<PointT>::Ptr cloudFiltered(new pcl::PointCloud<PointT>);
        pcl::PassThrough<PointT> pass;
        pass.setInputCloud(cloudTarget);
        pass.setFilterFieldName(fields[d]);
        pass.setFilterLimits(limits[2 * d], limits[2 * d + 1]);
        pass.filter(*cloudFiltered);
        cloudTarget = cloudFiltered;
      }
      ope::ObjectSegmentationPlane objSegPlane;
      const bool isPlane = objSegPlane.getSegmentedObjectsOnPlane(cloudTarget, clusters, cloudPlane);
      if (!isPlane) { std::printf("segment no plane (status %d)\n", objSegPlane.lastResult().status); return 5; }
      std::printf("segment plane %zu\n", cloudPlane->size());
      std::printf("segment clusters %zu sizes", clusters.size());
      for (const auto &c : clusters) std::printf(" %zu", c->size());
      std::printf("\n");
    }
    for (size_t k = 1; !segment && !frame && k < files.size(); ++k) {
      clusters.emplace_back(new pcl::PointCloud<PointT>);
      if (pcl::io::loadPCDFile(files[k], *clusters.back()) != 0) return 3;
    }
    double fitnessScore = 10.0, alignedStrength = 0.0;
    int selected = -1;
    pcl::Matrix4f pose = pcl::Matrix4f::Identity();
    if (candidates == 1) {
      pose = poseEstimator.estimateFinalPoseCandidates(cloudSource, clusters, fitnessScore, alignedStrength, selected);
    } else {
      for (size_t i = 0; i < clusters.size(); ++i) {   // rosinterface.cpp:244-259
        *cloudSource = *cloudSourceOriginal;
        if (!clusters[i]->empty()) pose = poseEstimator.estimateFinalPose(cloudSource, clusters[i], fitnessScore, alignedStrength);
        if (fitnessScore < 0.0001 || alignedStrength > 0.4) { selected = (int)i; break; }
      }
    }
    std::printf("candidates selected %d clusters %zu\n", selected, clusters.size());
    print_frame(1, pose, fitnessScore, alignedStrength);
  }
  for (size_t k = 1; !candidates && k < files.size(); ++k) {
    pcl::PointCloud<PointT>::Ptr cloudTargetSeg(new pcl::PointCloud<PointT>);
    if (pcl::io::loadPCDFile(files[k], *cloudTargetSeg) != 0) return 3;
    double fitnessScore = 10.0, alignedStrength = 0.0;
    // later frames hand over the source as the previous call left it (rosinterface.cpp:285: cloudSource is not reset)
    const pcl::Matrix4f pose = poseEstimator.estimateFinalPose(cloudSource, cloudTargetSeg, fitnessScore, alignedStrength);
    print_frame(k, pose, fitnessScore, alignedStrength);
  }
  const std::string out = files[1] + ".aligned.pcd";
  if (pcl::io::savePCDFile(out, *cloudSource, true) != 0) return 4;
  std::printf("aligned %s\n", out.c_str());
  return 0;
}
