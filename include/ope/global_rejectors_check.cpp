// global_rejectors_check.cpp — compat::registration::CorrespondenceRejectorMedianDistance, CorrespondenceRejectorOneToOne and
// CorrespondenceRejectorVarTrimmed stand-alone and through IterativeClosestPoint::align, for tests/test_gpu_global_rejectors_facade.py:
//
//   global_rejectors_check <pairs.txt> <source.pcd> <target.pcd> [--factor F] [--min-ratio R] [--iterations K]
//
// pairs.txt: one correspondence per line, `index_query index_match distance` (distance as C99 hex).  Prints, floats as C99 hex (%a),
// matrices column-major, hashes FNV-1a over the int32 arrays:
//   median remaining <n> query <h> match <h> distance <median>                 getRemainingCorrespondences at factor F (default 0.8)
//   one-to-one remaining <n> query <h> match <h>
//   trimmed remaining <n> query <h> match <h> distance <trimmed> factor <ratio>  at min ratio R (default 0.3)
//   align converged <c> iterations <i> pairs <n> query <h> match <h> median <d> T <16>
//                                      IterativeClosestPoint with [one-to-one, median F] added, K iterations (default 5)
//   wrong-order converged <c> iterations <i> T <16>                            a surface-normal rejector added AFTER the median one
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

static void print16(const pcl::Matrix4f &m) {
  std::printf(" T");
  for (int i = 0; i < 16; ++i) std::printf(" %a", (double)m.m[i]);
  std::printf("\n");
}

template <class Get> static uint64_t fnv(const pcl::Correspondences &c, Get get) {
  uint64_t h = 1469598103934665603ull;
  for (const pcl::Correspondence &e : c) {
    const int32_t w = get(e);
    const unsigned char *b = reinterpret_cast<const unsigned char *>(&w);
    for (int k = 0; k < 4; ++k) { h ^= b[k]; h *= 1099511628211ull; }
  }
  return h;
}
static void print_remaining(const char *tag, const pcl::Correspondences &c) {
  std::printf("%s remaining %zu query %016" PRIx64 " match %016" PRIx64, tag, c.size(),
              fnv(c, [](const pcl::Correspondence &e) { return (int32_t)e.index_query; }),
              fnv(c, [](const pcl::Correspondence &e) { return (int32_t)e.index_match; }));
}

int main(int argc, char **argv) {
  std::vector<std::string> files;
  double factor = 0.8, min_ratio = 0.3;
  int iterations = 5;
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--factor") && i + 1 < argc) factor = std::atof(argv[++i]);
    else if (!std::strcmp(argv[i], "--min-ratio") && i + 1 < argc) min_ratio = std::atof(argv[++i]);
    else if (!std::strcmp(argv[i], "--iterations") && i + 1 < argc) iterations = std::atoi(argv[++i]);
    else files.push_back(argv[i]);
  }
  if (files.size() != 3) {
    std::fprintf(stderr, "usage: %s <pairs.txt> <source.pcd> <target.pcd> [--factor F] [--min-ratio R] [--iterations K]\n", argv[0]);
    return 2;
  }
  std::shared_ptr<pcl::Correspondences> pairs(new pcl::Correspondences);
  {
    FILE *f = std::fopen(files[0].c_str(), "r");
    if (!f) return 3;
    int q, m;
    double d;
    while (std::fscanf(f, "%d %d %la", &q, &m, &d) == 3) {
      pcl::Correspondence c;
      c.index_query = q; c.index_match = m; c.distance = (float)d;
      pairs->push_back(c);
    }
    std::fclose(f);
  }
  Cloud::Ptr source(new Cloud), target(new Cloud);
  if (pcl::io::loadPCDFile(files[1], *source) != 0 || pcl::io::loadPCDFile(files[2], *target) != 0) return 3;

  // stand-alone, as the reference's block would call them (poseestimator.cpp:250-292)
  pcl::Correspondences remaining;
  pcl::registration::CorrespondenceRejectorMedianDistance median;
  median.setMedianFactor(factor);
  median.setInputCorrespondences(pairs);
  median.getCorrespondences(remaining);
  print_remaining("median", remaining);
  std::printf(" distance %a\n", median.getMedianDistance());

  pcl::registration::CorrespondenceRejectorOneToOne oneToOne;
  oneToOne.getRemainingCorrespondences(*pairs, remaining);
  print_remaining("one-to-one", remaining);
  std::printf("\n");

  pcl::registration::CorrespondenceRejectorVarTrimmed trimmed;
  trimmed.setMinRatio(min_ratio);
  trimmed.getRemainingCorrespondences(*pairs, remaining);
  print_remaining("trimmed", remaining);
  std::printf(" distance %a factor %a\n", trimmed.getTrimmedDistance(), trimmed.getTrimFactor());

  // inside the loop: [one to one, median], in the order added
  {
    pcl::registration::CorrespondenceRejectorOneToOne::Ptr r1(new pcl::registration::CorrespondenceRejectorOneToOne);
    pcl::registration::CorrespondenceRejectorMedianDistance::Ptr r2(new pcl::registration::CorrespondenceRejectorMedianDistance);
    r2->setMedianFactor(factor);
    pcl::IterativeClosestPoint<PointT, PointT> icp;
    icp.setInputSource(source);
    icp.setInputTarget(target);
    icp.setMaximumIterations(iterations);
    icp.addCorrespondenceRejector(r1);
    icp.addCorrespondenceRejector(r2);
    Cloud aligned;
    icp.align(aligned);
    const pcl::Correspondences last = icp.getCorrespondences();
    std::printf("align converged %d iterations %d pairs %zu query %016" PRIx64 " match %016" PRIx64 " median %a", icp.hasConverged() ? 1 : 0,
                icp.getNumberOfIterations(), last.size(), fnv(last, [](const pcl::Correspondence &e) { return (int32_t)e.index_query; }),
                fnv(last, [](const pcl::Correspondence &e) { return (int32_t)e.index_match; }), r2->getMedianDistance());
    print16(icp.getFinalTransformation());
  }
  // a pointwise rejector behind a global one cannot be honoured: align() says so and does not converge
  {
    pcl::registration::CorrespondenceRejectorMedianDistance::Ptr r1(new pcl::registration::CorrespondenceRejectorMedianDistance);
    pcl::registration::CorrespondenceRejectorSurfaceNormal::Ptr r2(new pcl::registration::CorrespondenceRejectorSurfaceNormal);
    pcl::IterativeClosestPoint<PointT, PointT> icp;
    icp.setInputSource(source);
    icp.setInputTarget(target);
    icp.setMaximumIterations(iterations);
    icp.addCorrespondenceRejector(r1);
    icp.addCorrespondenceRejector(r2);
    Cloud aligned;
    icp.align(aligned);
    std::printf("wrong-order converged %d iterations %d", icp.hasConverged() ? 1 : 0, icp.getNumberOfIterations());
    print16(icp.getFinalTransformation());
  }
  return 0;
}
