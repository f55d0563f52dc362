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
//   detect_and_localize --frame <model.pcd> <frame.pcd> --region-grow [--seed N] [--self-occluded]
// A frame whose objects no plane model separates (curved, many-faced, standing free): ope::SegmentationRegionGrow::getSegmentRegGrow
// (the z crop over [0, 1.2], normals with k = 30, region growing over them on the device), every cluster as --candidates takes
// them.  Prints `segment crop <n> sweeps <s>`, `segment clusters <n> sizes <s0> <s1> ...`, then the --candidates lines.
//
//   detect_and_localize --frame <model.pcd> <frame.pcd> --region-grow-rgb [--seed N] [--self-occluded]
// A frame whose objects differ from what they touch by colour alone (a coloured box against a wall, two flush parts):
// ope::SegmentationRegionGrow::getSegmentRegGrowRgb (the z crop over [0, 1.1], colour-based region growing on the device), every
// cluster as --candidates takes them.  Prints `segment crop <n> segments <s> absorbed <a>`, `segment clusters <n> sizes <s0> <s1>
// ...`, then the --candidates lines.
//
//   detect_and_localize --frame <model.pcd> <frame.pcd> --except-plane [--limits x0 x1 y0 y1 z0 z1] [--seed N] [--self-occluded]
// A frame without a single table (a floor, a wall, a shelf side): ope::ObjectSegmentationPlane::getSegmentedObjectsExceptPlane, its
// crop (getFiltered) set to the -l limits, planes peeled on the device until at most 30 % of the cropped points are left, the
// clusters of the remainder as --candidates takes them.  Prints `segment planes <k> sizes <c0> <c1> ... rest <m>`,
// `segment clusters <n> sizes <s0> <s1> ...`, then the --candidates lines.
//
//   ... --coarse sac-ia|prerejective|correspondences   (every mode but --depth)
// The coarse aligner of PoseEstimator::estimateCoarsePose: SAC-IA (the default, the reference's live code), the
// pcl::SampleConsensusPrerejective block the reference keeps commented out (BuildModel poseestimator.cpp:90-108; 50 000 iterations on
// the device), or its other commented block (:43-60, :111-113): FPFH matches, CorrespondenceRejectorSampleConsensus (10 000 iterations
// at 0.08) and the SVD over the remaining matches.  With correspondences the candidate loop and the tracker always run one
// estimateFinalPose at a time unless --correspondences-batch (below) is given; with prerejective they do unless
//   ... --coarse-batch   (every mode but --depth, --track and --track-loop)
// is given: PoseEstimator::setCoarseBatch(true), so --candidates (and --segment, --frame) with --coarse prerejective check all
// clusters in one ope_final_pose_batch_prerejective call.  Without the flag every mode prints what it printed before.
//   ... --device-draws   (with --coarse prerejective --coarse-batch)
// PoseEstimator::setCoarseDeviceDraws(true): that call makes its draws on the device; it prints the same lines.  Exit status 2
// without --coarse prerejective --coarse-batch.
//   ... --correspondences-batch   (with --coarse correspondences; not with --track or --track-loop)
// PoseEstimator::setCorrespondencesBatch(true): --candidates (and --segment, --frame) with --coarse correspondences check all clusters
// in one ope_final_pose_batch_correspondences call.  Exit status 2 without --coarse correspondences.  --coarse-batch does not touch
// this aligner: with it alone the loop still runs.
//
//   ... --fine-rejector median:<factor>|one-to-one|trimmed:<min_ratio>   (every mode but --depth; repeatable)
// PoseEstimator::addFineRejector: the rejectors estimateFinePose's list keeps commented out (poseestimator.cpp:250-292; the reference's
// literals are median:0.8 and trimmed:0.3), applied inside the fine ICP in the order given on the command line, behind the
// surface-normal rejector.  With the flag the candidate loop and the tracker run one estimateFinalPose at a time (the batched and
// tracked entry points take no list from the context).  Exit status 2 for another name or a value that does not parse.
//   ... --fine-rejector-batch   (with --fine-rejector; not with --track or --track-loop)
// PoseEstimator::setFineRejectorBatch(true): --candidates (and --segment, --frame) with the SAC-IA coarse stage check all clusters
// in one ope_final_pose_batch_rejectors call, the list applied inside the batched ICP kernel.  Exit status 2 without
// --fine-rejector.  Without the flag every mode prints what it printed before.
//
//   ... --recognise <train_dir>   (with --candidates, --candidates-loop, --segment or --frame)
// Before the pose stage, ope::ObjectDetection::getObjectNames over every cluster in one call against the table under <train_dir>
// (training_data.list / training_data.f32).  Prints `recognise <i> <name> <distance>` per cluster: the name getObjectName gives
// and the distance it compares with 120 (the reference's "distance of 1-NN", read from neighbour [1]).  Nothing else changes.
//
//   detect_and_localize --track <model.pcd> --frame <a.pcd> [<b.pcd> ...] [--frame ...] [--seed N] [--self-occluded] [--time]
//   detect_and_localize --track-loop <model.pcd> --frame ... (same)
// DetectAndLocalize's per-frame policy (rosinterface.cpp:226-313) over a sequence of camera frames, one --frame per frame with
// that frame's clusters (none: an empty frame).  --track: ope::ObjectTracker::localize (the gate and the gated pose on the
// device); --track-loop: ObjectTracker::localizeLoop (host compute3DCentroid and estimateFinalPose, as the reference writes it).
// Per frame: `track frame <k> branch <b> selected <i> clusters <n>`, then the `frame ...` line; --time adds `time frame <k> ms <t>`
// (host clock around the synchronised call).
//
//   detect_and_localize --depth <model.pcd> <d0.pgm> [<d1.pgm> ...] [--sensor kinect|astra|euclid] [--limits x0 x1 y0 y1 z0 z1] [--seed N] [--time]
//   detect_and_localize --depth-host <model.pcd> <d0.pgm> ... (same)
// The body of the reference's per-frame loop from the sensor's depth image on (rosinterface.cpp:422, 212-313), one 16-bit PGM per
// frame.  --depth: ope::DataGrabber::rgbd2PclDevice (conversion and the -l crop on the device), getSegmentedObjectsOnPlane on
// that device frame, ObjectTracker::localize.  --depth-host: DataGrabber::rgbd2Pcl (the reference's loop on the host, no device
// code), the three pcl::PassThrough, the upload inside getSegmentedObjectsOnPlane — the same frames the way they arrived before
// the device ingest.  Per frame: `depth frame <k> points <n> plane <n> clusters <n> sizes ...`, then the --track lines; --time adds
// `time frame <k> ms <t>` over the whole frame and `time ingest frame <k> ms <t> segment <t>`: until the cropped frame is ready
// (--depth: on the device, synchronised; --depth-host: on the host), and getSegmentedObjectsOnPlane (--depth-host: with its upload).
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <chrono>

#include "data_grabber.hpp"
#include "object_detection.hpp"
#include "object_segmentation_plane.hpp"
#include "object_tracker.hpp"
#include "pcd_io.hpp"
#include "pose_estimator.hpp"
#include "segmentation_region_grow.hpp"

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

// --fine-rejector's value: false for an unknown name or a number that does not parse
static bool parse_fine_rejector(const char *v, ope::PoseEstimator &pe) {
  namespace reg = pcl::registration;
  char *end = nullptr;
  if (!std::strcmp(v, "one-to-one")) { pe.addFineRejector(reg::CorrespondenceRejector::Ptr(new reg::CorrespondenceRejectorOneToOne)); return true; }
  if (!std::strncmp(v, "median:", 7)) {
    const double f = std::strtod(v + 7, &end);
    if (end != v + 7 && *end == 0) {
      reg::CorrespondenceRejectorMedianDistance::Ptr r(new reg::CorrespondenceRejectorMedianDistance);
      r->setMedianFactor(f);
      pe.addFineRejector(r);
      return true;
    }
  }
  if (!std::strncmp(v, "trimmed:", 8)) {
    const double f = std::strtod(v + 8, &end);
    if (end != v + 8 && *end == 0) {
      reg::CorrespondenceRejectorVarTrimmed::Ptr r(new reg::CorrespondenceRejectorVarTrimmed);
      r->setMinRatio(f);
      pe.addFineRejector(r);
      return true;
    }
  }
  std::fprintf(stderr, "--fine-rejector takes median:<factor>, one-to-one or trimmed:<min_ratio>\n");
  return false;
}

// --coarse's value: false for an unknown name
static bool parse_coarse(const char *v, ope::PoseEstimator::CoarseMethod &m) {
  if (!std::strcmp(v, "sac-ia")) { m = ope::PoseEstimator::COARSE_SAC_IA; return true; }
  if (!std::strcmp(v, "prerejective")) { m = ope::PoseEstimator::COARSE_PREREJECTIVE; return true; }
  if (!std::strcmp(v, "correspondences")) { m = ope::PoseEstimator::COARSE_CORRESPONDENCES; return true; }
  std::fprintf(stderr, "--coarse takes sac-ia, prerejective or correspondences\n");
  return false;
}

// --track / --track-loop
static int track_main(int argc, char **argv) {
  int mode = 0;   // 1: --track, 2: --track-loop
  std::string model_path;
  std::vector<std::vector<std::string>> frames;
  uint64_t seed = 1;
  bool self_occluded = false, timed = false;
  ope::PoseEstimator::CoarseMethod coarse = ope::PoseEstimator::COARSE_SAC_IA;
  std::vector<const char *> fine_rejectors;
  for (int i = 1; i < argc; ++i) {
    if ((!std::strcmp(argv[i], "--track") || !std::strcmp(argv[i], "--track-loop")) && i + 1 < argc) {
      mode = !std::strcmp(argv[i], "--track") ? 1 : 2;
      model_path = argv[++i];
    } else if (!std::strcmp(argv[i], "--frame")) frames.emplace_back();
    else if (!std::strcmp(argv[i], "--seed") && i + 1 < argc) seed = std::strtoull(argv[++i], nullptr, 10);
    else if (!std::strcmp(argv[i], "--coarse") && i + 1 < argc) { if (!parse_coarse(argv[++i], coarse)) return 2; }
    else if (!std::strcmp(argv[i], "--self-occluded")) self_occluded = true;
    else if (!std::strcmp(argv[i], "--fine-rejector") && i + 1 < argc) fine_rejectors.push_back(argv[++i]);
    else if (!std::strcmp(argv[i], "--coarse-batch")) { std::fprintf(stderr, "--coarse-batch does not go with --track or --track-loop\n"); return 2; }
    else if (!std::strcmp(argv[i], "--device-draws")) { std::fprintf(stderr, "--device-draws does not go with --track or --track-loop\n"); return 2; }
    else if (!std::strcmp(argv[i], "--correspondences-batch")) { std::fprintf(stderr, "--correspondences-batch does not go with --track or --track-loop\n"); return 2; }
    else if (!std::strcmp(argv[i], "--fine-rejector-batch")) { std::fprintf(stderr, "--fine-rejector-batch does not go with --track or --track-loop\n"); return 2; }
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
  tracker.estimator().setCoarseMethod(coarse);
  tracker.estimator().setUseSelfOccludedRejector(self_occluded);
  for (const char *v : fine_rejectors)
    if (!parse_fine_rejector(v, tracker.estimator())) return 2;
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

// --depth / --depth-host
static int depth_main(int argc, char **argv) {
  int mode = 0;   // 1: --depth, 2: --depth-host
  std::vector<std::string> files;
  std::string sensor = "kinect";
  uint64_t seed = 1;
  bool timed = false, limited = false;
  float limits[6] = {-FLT_MAX, FLT_MAX, -FLT_MAX, FLT_MAX, -FLT_MAX, FLT_MAX};
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--depth")) mode = 1;
    else if (!std::strcmp(argv[i], "--depth-host")) mode = 2;
    else if (!std::strcmp(argv[i], "--sensor") && i + 1 < argc) sensor = argv[++i];
    else if (!std::strcmp(argv[i], "--seed") && i + 1 < argc) seed = std::strtoull(argv[++i], nullptr, 10);
    else if (!std::strcmp(argv[i], "--time")) timed = true;
    else if (!std::strcmp(argv[i], "--limits") && i + 6 < argc) { limited = true; for (int d = 0; d < 6; ++d) limits[d] = std::strtof(argv[++i], nullptr); }
    else files.push_back(argv[i]);
  }
  const bool euclid = sensor == "euclid", kinect = sensor == "kinect", astra = sensor == "astra";
  if (!mode || files.size() < 2 || !(euclid || kinect || astra)) {
    std::fprintf(stderr, "usage: %s --depth|--depth-host <model.pcd> <d0.pgm> [<d1.pgm> ...] [--sensor kinect|astra|euclid] [--limits ...] [--seed N] [--time]\n", argv[0]);
    return 2;
  }
  typedef ope::PoseEstimator::PointT PointT;
  pcl::PointCloud<PointT> model;
  if (pcl::io::loadPCDFile(files[0], model) != 0) return 3;
  ope::DataGrabber dataGrabber(euclid, kinect, astra);   // rosinterface.cpp:70
  ope::ObjectTracker tracker(model);
  tracker.estimator().setSacIaSeed(seed);
  const float lo[3] = {limits[0], limits[2], limits[4]}, hi[3] = {limits[1], limits[3], limits[5]};
  double fitnessScore = 10.0, alignedStrength = 0.0;
  for (size_t k = 1; k < files.size(); ++k) {
    ope::DepthImage imageDepth;
    if (ope::io::loadPGM(files[k], imageDepth) != 0) return 3;
    ope_ctx *ctx = pcl::default_context();
    if (ctx) ope_ctx_sync(ctx);
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<pcl::PointCloud<PointT>::Ptr> clusters;
    pcl::PointCloud<PointT>::Ptr cloudPlane;
    ope::ObjectSegmentationPlane objSegPlane;
    size_t points = 0;
    bool isPlane = false;
    auto t1 = t0;
    if (mode == 1) {
      auto frame = dataGrabber.rgbd2PclDevice(imageDepth, limited ? lo : nullptr, limited ? hi : nullptr);
      if (!frame->h) return 4;
      points = ope_cloud_size(frame->h);
      t1 = std::chrono::steady_clock::now();   // (ope_depth_to_cloud returns synchronised)
      isPlane = objSegPlane.getSegmentedObjectsOnPlane(*frame, clusters, cloudPlane);
    } else {
      pcl::PointCloud<PointT>::Ptr cloudTarget = dataGrabber.rgbd2Pcl(imageDepth);   // rosinterface.cpp:422
      const char *fields[3] = {"x", "y", "z"};
      for (int d = 0; limited && d < 3; ++d) {   // ProcessingPcd::getPassThrough (processingpcd.cpp:13-33)
        pcl::PointCloud<PointT>::Ptr cloudFiltered(new pcl::PointCloud<PointT>);
        pcl::PassThrough<PointT> pass;
        pass.setInputCloud(cloudTarget);
        pass.setFilterFieldName(fields[d]);
        pass.setFilterLimits(limits[2 * d], limits[2 * d + 1]);
        pass.filter(*cloudFiltered);
        cloudTarget = cloudFiltered;
      }
      points = cloudTarget->size();
      t1 = std::chrono::steady_clock::now();
      isPlane = objSegPlane.getSegmentedObjectsOnPlane(cloudTarget, clusters, cloudPlane);
    }
    const auto t2 = std::chrono::steady_clock::now();
    if (!isPlane) clusters.clear();   // (no table in this frame: nothing to localize against)
    const pcl::Matrix4f pose = tracker.localize(clusters, fitnessScore, alignedStrength);
    if (ctx) ope_ctx_sync(ctx);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const ope::PoseEstimator &e = tracker.estimator();
    std::printf("depth frame %zu points %zu plane %zu clusters %zu sizes", k, points, isPlane ? cloudPlane->size() : (size_t)0, clusters.size());
    for (const auto &c : clusters) std::printf(" %zu", c->size());
    std::printf("\n");
    std::printf("track frame %zu branch %s selected %d clusters %zu\n", k, branch_name(tracker.lastBranch()), tracker.lastSelected(), clusters.size());
    if (timed) {
      std::printf("time frame %zu ms %.4f\n", k, ms);
      std::printf("time ingest frame %zu ms %.4f segment %.4f\n", k, std::chrono::duration<double, std::milli>(t1 - t0).count(),
                  std::chrono::duration<double, std::milli>(t2 - t1).count());
    }
    std::printf("frame %zu fitness %.12g strength %.12g coarse_calls %d icp_iterations %d", k, fitnessScore, alignedStrength, e.coarseCalls(),
                e.lastIcpIterations());
    print16("final", pose);
    print16("coarse", e.lastCoarsePose());
    print16("fine", e.lastFinePose());
    print16("rigid", e.lastRigidModelPose());
    std::printf("\n");
  }
  return 0;
}

int main(int argc, char **argv) {
  for (int i = 1; i < argc; ++i)
    if (!std::strcmp(argv[i], "--depth") || !std::strcmp(argv[i], "--depth-host")) return depth_main(argc, argv);
  for (int i = 1; i < argc; ++i)
    if (!std::strcmp(argv[i], "--track") || !std::strcmp(argv[i], "--track-loop")) return track_main(argc, argv);
  std::vector<std::string> files;
  uint64_t seed = 1;
  bool self_occluded = false;
  int candidates = 0;   // 1: estimateFinalPoseCandidates, 2: the reference's loop
  bool segment = false; // --segment: the clusters come from getClusters over the one scene file (the non-plane cloud)
  bool frame = false;   // --frame: the clusters come from getSegmentedObjectsOnPlane over the one scene file (a camera frame)
  bool except_plane = false;   // --except-plane (with --frame): from getSegmentedObjectsExceptPlane instead
  bool region_grow = false;    // --region-grow (with --frame): from SegmentationRegionGrow::getSegmentRegGrow instead
  bool region_grow_rgb = false;   // --region-grow-rgb (with --frame): from SegmentationRegionGrow::getSegmentRegGrowRgb instead
  std::string recognise;       // --recognise <train_dir>: name every cluster before the pose stage
  ope::PoseEstimator::CoarseMethod coarse = ope::PoseEstimator::COARSE_SAC_IA;   // --coarse
  bool coarse_batch = false;   // --coarse-batch
  bool device_draws = false;   // --device-draws
  bool correspondences_batch = false;   // --correspondences-batch
  std::vector<const char *> fine_rejectors;   // --fine-rejector, in the order given
  bool fine_rejector_batch = false;           // --fine-rejector-batch
  float limits[6] = {-FLT_MAX, FLT_MAX, -FLT_MAX, FLT_MAX, -FLT_MAX, FLT_MAX};
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--seed") && i + 1 < argc) seed = std::strtoull(argv[++i], nullptr, 10);
    else if (!std::strcmp(argv[i], "--coarse") && i + 1 < argc) { if (!parse_coarse(argv[++i], coarse)) return 2; }
    else if (!std::strcmp(argv[i], "--coarse-batch")) coarse_batch = true;
    else if (!std::strcmp(argv[i], "--device-draws")) device_draws = true;
    else if (!std::strcmp(argv[i], "--correspondences-batch")) correspondences_batch = true;
    else if (!std::strcmp(argv[i], "--fine-rejector") && i + 1 < argc) fine_rejectors.push_back(argv[++i]);
    else if (!std::strcmp(argv[i], "--fine-rejector-batch")) fine_rejector_batch = true;
    else if (!std::strcmp(argv[i], "--recognise") && i + 1 < argc) recognise = argv[++i];
    else if (!std::strcmp(argv[i], "--self-occluded")) self_occluded = true;
    else if (!std::strcmp(argv[i], "--candidates")) candidates = 1;
    else if (!std::strcmp(argv[i], "--candidates-loop")) candidates = 2;
    else if (!std::strcmp(argv[i], "--segment")) { segment = true; candidates = 1; }
    else if (!std::strcmp(argv[i], "--frame")) { frame = true; candidates = 1; }
    else if (!std::strcmp(argv[i], "--except-plane")) except_plane = true;
    else if (!std::strcmp(argv[i], "--region-grow")) region_grow = true;
    else if (!std::strcmp(argv[i], "--region-grow-rgb")) region_grow_rgb = true;
    else if (!std::strcmp(argv[i], "--limits") && i + 6 < argc) { for (int d = 0; d < 6; ++d) limits[d] = std::strtof(argv[++i], nullptr); }
    else files.push_back(argv[i]);
  }
  if (correspondences_batch && coarse != ope::PoseEstimator::COARSE_CORRESPONDENCES) {
    std::fprintf(stderr, "--correspondences-batch goes with --coarse correspondences\n");
    return 2;
  }
  if (device_draws && !(coarse == ope::PoseEstimator::COARSE_PREREJECTIVE && coarse_batch)) {
    std::fprintf(stderr, "--device-draws goes with --coarse prerejective --coarse-batch\n");
    return 2;
  }
  if (fine_rejector_batch && fine_rejectors.empty()) { std::fprintf(stderr, "--fine-rejector-batch goes with --fine-rejector\n"); return 2; }
  if (except_plane && !frame) { std::fprintf(stderr, "--except-plane goes with --frame\n"); return 2; }
  if (region_grow && (!frame || except_plane)) { std::fprintf(stderr, "--region-grow goes with --frame and without --except-plane\n"); return 2; }
  if (region_grow_rgb && (!frame || except_plane || region_grow)) {
    std::fprintf(stderr, "--region-grow-rgb goes with --frame and without --except-plane and --region-grow\n");
    return 2;
  }
  if (!recognise.empty() && !candidates) { std::fprintf(stderr, "--recognise goes with --candidates, --candidates-loop, --segment or --frame\n"); return 2; }
  if (files.size() < 2) { std::fprintf(stderr, "usage: %s <model.pcd> <scene.pcd> [more scenes] [--seed N] [--self-occluded] [--candidates | --candidates-loop | --segment | --frame]\n", argv[0]); return 2; }
  typedef ope::PoseEstimator::PointT PointT;
  pcl::PointCloud<PointT>::Ptr cloudSourceOriginal(new pcl::PointCloud<PointT>), cloudSource(new pcl::PointCloud<PointT>);
  if (pcl::io::loadPCDFile(files[0], *cloudSourceOriginal) != 0) return 3;   // rosinterface.cpp:80
  *cloudSource = *cloudSourceOriginal;
  ope::PoseEstimator poseEstimator;
  poseEstimator.setSacIaSeed(seed);
  poseEstimator.setCoarseMethod(coarse);
  poseEstimator.setCoarseBatch(coarse_batch);
  poseEstimator.setCoarseDeviceDraws(device_draws);
  poseEstimator.setCorrespondencesBatch(correspondences_batch);
  poseEstimator.setUseSelfOccludedRejector(self_occluded);
  poseEstimator.setFineRejectorBatch(fine_rejector_batch);
  for (const char *v : fine_rejectors)
    if (!parse_fine_rejector(v, poseEstimator)) return 2;
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
    if (frame && except_plane) {
      pcl::PointCloud<PointT>::Ptr cloudTarget(new pcl::PointCloud<PointT>);
      if (segment || files.size() != 2 || pcl::io::loadPCDFile(files[1], *cloudTarget) != 0) return 3;
      ope::ObjectSegmentationPlane objSegPlane;
      objSegPlane.setFilterLimits(limits[0], limits[1], limits[2], limits[3], limits[4], limits[5]);
      clusters = objSegPlane.getSegmentedObjectsExceptPlane(cloudTarget);
      if (objSegPlane.deviceFailed()) return 5;
      std::printf("segment planes %d sizes", objSegPlane.lastPeel().n_planes);
      for (int32_t c : objSegPlane.lastPeelCounts()) std::printf(" %d", c);
      std::printf(" rest %d\n", objSegPlane.lastPeel().n_rest);
      std::printf("segment clusters %zu sizes", clusters.size());
      for (const auto &c : clusters) std::printf(" %zu", c->size());
      std::printf("\n");
    } else if (frame && region_grow) {
      pcl::PointCloud<PointT>::Ptr cloudTarget(new pcl::PointCloud<PointT>);
      if (segment || files.size() != 2 || pcl::io::loadPCDFile(files[1], *cloudTarget) != 0) return 3;
      ope::SegmentationRegionGrow segRegGrow;
      segRegGrow.getSegmentRegGrow(cloudTarget);
      if (segRegGrow.deviceFailed()) return 5;
      clusters = segRegGrow.getClusters();
      std::printf("segment crop %zu sweeps %lld\n", segRegGrow.lastCropSize(), (long long)segRegGrow.lastStats().sweeps);
      std::printf("segment clusters %zu sizes", clusters.size());
      for (const auto &c : clusters) std::printf(" %zu", c->size());
      std::printf("\n");
    } else if (frame && region_grow_rgb) {
      pcl::PointCloud<PointT>::Ptr cloudTarget(new pcl::PointCloud<PointT>);
      if (segment || files.size() != 2 || pcl::io::loadPCDFile(files[1], *cloudTarget) != 0) return 3;
      ope::SegmentationRegionGrow segRegGrow;
      segRegGrow.getSegmentRegGrowRgb(cloudTarget);
      if (segRegGrow.deviceFailed()) return 5;
      clusters = segRegGrow.getClusters();
      std::printf("segment crop %zu segments %lld absorbed %lld\n", segRegGrow.lastCropSize(), (long long)segRegGrow.lastRgbStats().segments,
                  (long long)segRegGrow.lastRgbStats().regions_absorbed);
      std::printf("segment clusters %zu sizes", clusters.size());
      for (const auto &c : clusters) std::printf(" %zu", c->size());
      std::printf("\n");
    } else if (frame) {
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
    if (!recognise.empty()) {
      ope::ObjectDetection objDetection;
      if (!objDetection.loadTrainData(recognise)) return 6;
      std::vector<std::string> names;
      std::vector<float> dist;
      if (!clusters.empty() && !objDetection.getObjectNames(clusters, names, &dist)) return 5;
      for (size_t i = 0; i < names.size(); ++i) std::printf("recognise %zu %s %.9g\n", i, names[i].c_str(), (double)dist[i]);
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
