// corr_sac_check.cpp — compat::registration::CorrespondenceEstimation over FPFH rows, CorrespondenceRejectorSampleConsensus and
// ope::PoseEstimator::COARSE_CORRESPONDENCES from files, for tests/test_gpu_corr_sac_facade.py:
//
//   corr_sac_check <model.pcd> <scene.pcd> [--seed N] [--iterations H] [--threshold T]
//
// Key points and FPFH rows of both clouds as PoseEstimator::getFpfhFeatures makes them (poseestimator.cpp:110-128).  Prints, floats
// as C99 hex (%a), matrices column-major, hashes FNV-1a over the int32 / float32 arrays:
//   keys <ns> <nt>
//   matches <n> query <h> match <h> distance <h>                              determineCorrespondences (BuildModel poseestimator.cpp:43-47)
//   remaining <n> query <h> match <h> found <f> iterations <i> T <16>         the rejector (:49-60) with H iterations (default 10000) at
//                                                                            T (default 0.08); T = getBestTransformation()
//   svd T <16>                                                                TransformationEstimationSVD over the remaining (:111-113)
//   estimator sac-ia T <16>                                                   PoseEstimator::estimateCoarsePose, the default method, seed N
//   estimator correspondences T <16>                                          ... after setCoarseMethod(COARSE_CORRESPONDENCES)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "pcd_io.hpp"
#include "pose_estimator.hpp"

namespace pcl = ope::compat;
typedef ope::PoseEstimator::PointT PointT;
typedef pcl::PointCloud<PointT> Cloud;
typedef pcl::PointCloud<pcl::FPFHSignature33> FeatureCloud;

static void print16(const pcl::Matrix4f &m) {
  std::printf(" T");
  for (int i = 0; i < 16; ++i) std::printf(" %a", (double)m.m[i]);
  std::printf("\n");
}

template <class Get> static uint64_t fnv(const pcl::Correspondences &c, Get get) {
  uint64_t h = 1469598103934665603ull;
  for (const pcl::Correspondence &e : c) {
    const auto w = get(e);
    static_assert(sizeof w == 4, "four bytes per entry");
    const unsigned char *b = reinterpret_cast<const unsigned char *>(&w);
    for (int k = 0; k < 4; ++k) { h ^= b[k]; h *= 1099511628211ull; }
  }
  return h;
}

int main(int argc, char **argv) {
  std::vector<std::string> files;
  uint64_t seed = 1;
  int iterations = 10000;
  double threshold = 0.08;
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--seed") && i + 1 < argc) seed = std::strtoull(argv[++i], nullptr, 10);
    else if (!std::strcmp(argv[i], "--iterations") && i + 1 < argc) iterations = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--threshold") && i + 1 < argc) threshold = std::atof(argv[++i]);
    else files.push_back(argv[i]);
  }
  if (files.size() != 2) {
    std::fprintf(stderr, "usage: %s <model.pcd> <scene.pcd> [--seed N] [--iterations H] [--threshold T]\n", argv[0]);
    return 2;
  }
  Cloud::Ptr model(new Cloud), scene(new Cloud);
  if (pcl::io::loadPCDFile(files[0], *model) != 0 || pcl::io::loadPCDFile(files[1], *scene) != 0) return 3;

  ope::PoseEstimator features;
  Cloud::Ptr src(new Cloud(*model)), tgt(new Cloud(*scene)), srcKeys, tgtKeys;
  FeatureCloud::Ptr srcFeat, tgtFeat;
  features.getFpfhFeatures(src, srcFeat, srcKeys);
  features.getFpfhFeatures(tgt, tgtFeat, tgtKeys);
  std::printf("keys %zu %zu\n", src->size(), tgt->size());

  // BuildModel/src/poseestimator.cpp:43-47
  std::shared_ptr<pcl::Correspondences> correspondences(new pcl::Correspondences);
  pcl::registration::CorrespondenceEstimation<pcl::FPFHSignature33, pcl::FPFHSignature33> cest;
  cest.setInputSource(srcFeat);
  cest.setInputTarget(tgtFeat);
  cest.determineCorrespondences(*correspondences);
  std::printf("matches %zu query %016" PRIx64 " match %016" PRIx64 " distance %016" PRIx64 "\n", correspondences->size(),
              fnv(*correspondences, [](const pcl::Correspondence &e) { return (int32_t)e.index_query; }),
              fnv(*correspondences, [](const pcl::Correspondence &e) { return (int32_t)e.index_match; }),
              fnv(*correspondences, [](const pcl::Correspondence &e) { return (float)e.distance; }));

  // :49-60
  pcl::Correspondences correspondencesFiltered;
  pcl::registration::CorrespondenceRejectorSampleConsensus<PointT> rejector;
  rejector.setInputSource(src);
  rejector.setInputTarget(tgt);
  rejector.setMaximumIterations(iterations);
  rejector.setInlierThreshold(threshold);
  rejector.setInputCorrespondences(correspondences);
  rejector.getCorrespondences(correspondencesFiltered);
  std::printf("remaining %zu query %016" PRIx64 " match %016" PRIx64 " found %d iterations %d", correspondencesFiltered.size(),
              fnv(correspondencesFiltered, [](const pcl::Correspondence &e) { return (int32_t)e.index_query; }),
              fnv(correspondencesFiltered, [](const pcl::Correspondence &e) { return (int32_t)e.index_match; }), rejector.foundModel() ? 1 : 0,
              rejector.getNumberOfIterations());
  print16(rejector.getBestTransformation());

  // :111-113
  pcl::Matrix4f pose;
  pcl::registration::TransformationEstimationSVD<PointT, PointT> svd;
  svd.estimateRigidTransformation(*src, *tgt, correspondencesFiltered, pose);
  std::printf("svd");
  print16(pose);

  ope::PoseEstimator byDefault;
  byDefault.setSacIaSeed(seed);
  const pcl::Matrix4f poseDefault = byDefault.estimateCoarsePose(model, scene);
  std::printf("estimator sac-ia");
  print16(poseDefault);

  ope::PoseEstimator byMatches;
  byMatches.setSacIaSeed(seed);
  byMatches.setCoarseMethod(ope::PoseEstimator::COARSE_CORRESPONDENCES);
  const pcl::Matrix4f poseMatches = byMatches.estimateCoarsePose(model, scene);
  std::printf("estimator correspondences");
  print16(poseMatches);
  return byMatches.coarseCalls() == 1 && byDefault.coarseCalls() == 1 ? 0 : 4;
}
