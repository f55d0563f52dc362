// prerejective_check.cpp — compat::SampleConsensusPrerejective and ope::PoseEstimator::setCoarseMethod from files, for
// tests/test_gpu_prerejective_facade.py:
//
//   prerejective_check <model.pcd> <scene.pcd> [--seed N] [--iterations H]
//
// Key points and FPFH rows of both clouds as PoseEstimator::getFpfhFeatures makes them (poseestimator.cpp:110-128).  Prints, floats
// as C99 hex (%a) and matrices column-major:
//   keys <ns> <nt>
//   prerejective converged <c> iteration <i> inliers <n> error <e> T <16>    the reference's commented block (BuildModel
//                                                                            poseestimator.cpp:92-107) with H iterations (default 50000)
//   inliers <n> <h>                                                          getInliers(): FNV-1a of the int32 indices
//   sacia T <16>                                                             SAC-IA as estimateCoarsePose sets it up (:50-64), seed N
//   estimator sac-ia T <16>                                                  PoseEstimator::estimateCoarsePose, the default method
//   estimator prerejective T <16>                                            ... after setCoarseMethod(COARSE_PREREJECTIVE)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

int main(int argc, char **argv) {
  std::vector<std::string> files;
  uint64_t seed = 1;
  int iterations = 50000;
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--seed") && i + 1 < argc) seed = std::strtoull(argv[++i], nullptr, 10);
    else if (!std::strcmp(argv[i], "--iterations") && i + 1 < argc) iterations = std::atoi(argv[++i]);
    else files.push_back(argv[i]);
  }
  if (files.size() != 2) { std::fprintf(stderr, "usage: %s <model.pcd> <scene.pcd> [--seed N] [--iterations H]\n", argv[0]); return 2; }
  Cloud::Ptr model(new Cloud), scene(new Cloud);
  if (pcl::io::loadPCDFile(files[0], *model) != 0 || pcl::io::loadPCDFile(files[1], *scene) != 0) return 3;

  ope::PoseEstimator features;
  Cloud::Ptr src(new Cloud(*model)), tgt(new Cloud(*scene)), srcKeys, tgtKeys;
  FeatureCloud::Ptr srcFeat, tgtFeat;
  features.getFpfhFeatures(src, srcFeat, srcKeys);
  features.getFpfhFeatures(tgt, tgtFeat, tgtKeys);
  std::printf("keys %zu %zu\n", src->size(), tgt->size());

  // BuildModel/src/poseestimator.cpp:92-107
  Cloud::Ptr result(new Cloud);
  pcl::SampleConsensusPrerejective<PointT, PointT, pcl::FPFHSignature33> sacPreRej;
  sacPreRej.setInputSource(src);
  sacPreRej.setSourceFeatures(srcFeat);
  sacPreRej.setInputTarget(tgt);
  sacPreRej.setTargetFeatures(tgtFeat);
  sacPreRej.setMaximumIterations(iterations);
  sacPreRej.setNumberOfSamples(3);
  sacPreRej.setCorrespondenceRandomness(5);
  sacPreRej.setSimilarityThreshold(0.8f);
  sacPreRej.setMaxCorrespondenceDistance(0.15);
  sacPreRej.setInlierFraction(0.25f);
  sacPreRej.setSeed(seed);
  sacPreRej.align(*result);
  std::printf("prerejective converged %d iteration %d inliers %zu error %a", sacPreRej.hasConverged() ? 1 : 0, sacPreRej.getBestIteration(),
              sacPreRej.getInliers().size(), sacPreRej.getFitnessScore());
  print16(sacPreRej.getFinalTransformation());
  {
    uint64_t h = 1469598103934665603ull;
    for (int v : sacPreRej.getInliers()) {
      const int32_t w = v;
      const unsigned char *b = reinterpret_cast<const unsigned char *>(&w);
      for (int k = 0; k < 4; ++k) { h ^= b[k]; h *= 1099511628211ull; }
    }
    std::printf("inliers %zu %016" PRIx64 "\n", sacPreRej.getInliers().size(), h);
  }

  // DetectAndLocalize/src/poseestimator.cpp:50-64
  pcl::SampleConsensusInitialAlignment<PointT, PointT, pcl::FPFHSignature33> sacia;
  sacia.setInputSource(src);
  sacia.setInputTarget(tgt);
  sacia.setSourceFeatures(srcFeat);
  sacia.setTargetFeatures(tgtFeat);
  sacia.setMaximumIterations(400);
  sacia.setNumberOfSamples(5);
  sacia.setCorrespondenceRandomness(5);
  sacia.setMaxCorrespondenceDistance(0.05);
  sacia.setMinSampleDistance(0.01f);
  sacia.setSeed(seed);
  Cloud aligned;
  sacia.align(aligned);
  std::printf("sacia");
  print16(sacia.getFinalTransformation());

  ope::PoseEstimator byDefault;
  byDefault.setSacIaSeed(seed);
  const pcl::Matrix4f poseDefault = byDefault.estimateCoarsePose(model, scene);
  std::printf("estimator sac-ia");
  print16(poseDefault);

  ope::PoseEstimator prerejective;
  prerejective.setSacIaSeed(seed);
  prerejective.setCoarseMethod(ope::PoseEstimator::COARSE_PREREJECTIVE);
  const pcl::Matrix4f pose = prerejective.estimateCoarsePose(model, scene);
  std::printf("estimator prerejective");
  print16(pose);
  return prerejective.coarseCalls() == 1 && byDefault.coarseCalls() == 1 ? 0 : 4;
}
