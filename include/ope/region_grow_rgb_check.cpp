// region_grow_rgb_check.cpp — ope::SegmentationRegionGrow::getSegmentRegGrowRgb and compat::RegionGrowingRGB from a file, for
// tests/test_gpu_region_grow_rgb_facade.py:
//
//   region_grow_rgb_check <frame.pcd>
//
// Prints, point lists as an FNV-1a hash of their xyz bytes, <hc> as that of their rgb words and <hi> as that of their indices:
//   crop <n>                                     points the z crop over [0, 1.1] kept
//   regions <k> segments <s> pairs <p> homogeneous <h> absorbed <a>      getSegmentRegGrowRgb
//   region <i> <n> <h> <hc>                      ... each cluster (getClusters)
//   last <n> <h>                                 ... its return value
//   classes <k>                                  the same through PassThrough's indices and RegionGrowingRGB, as the reference
//   class <i> <n> <h> <hi>                       writes them (segmentationregiongrow.cpp:92-106), gathered from the input cloud
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pcd_io.hpp"
#include "segmentation_region_grow.hpp"

namespace pcl = ope::compat;
typedef ope::SegmentationRegionGrow::PointTSeg PointTSeg;
typedef pcl::PointCloud<PointTSeg> Cloud;

static uint64_t fnv(uint64_t h, const void *p, size_t n) {
  const unsigned char *b = static_cast<const unsigned char *>(p);
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}
static uint64_t hash_xyz(const Cloud &c) {
  uint64_t h = 1469598103934665603ull;
  for (const PointTSeg &p : c.points) { h = fnv(h, &p.x, 4); h = fnv(h, &p.y, 4); h = fnv(h, &p.z, 4); }
  return h;
}
static uint64_t hash_rgb(const Cloud &c) {
  uint64_t h = 1469598103934665603ull;
  for (const PointTSeg &p : c.points) h = fnv(h, &p.rgb, 4);
  return h;
}

int main(int argc, char **argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s <frame.pcd>\n", argv[0]); return 2; }
  Cloud::Ptr frame(new Cloud);
  if (pcl::io::loadPCDFile(argv[1], *frame) != 0) return 3;
  ope::SegmentationRegionGrow seg;
  Cloud::Ptr last = seg.getSegmentRegGrowRgb(frame);
  if (seg.deviceFailed()) return 5;
  const auto &all = seg.getClusters();
  if (all.size() != seg.deviceClusters().size()) return 6;
  const ope_region_rgb_stats &st = seg.lastRgbStats();
  std::printf("crop %zu\n", seg.lastCropSize());
  std::printf("regions %zu segments %lld pairs %lld homogeneous %lld absorbed %lld\n", all.size(), (long long)st.segments, (long long)st.segment_pairs,
              (long long)st.homogeneous_regions, (long long)st.regions_absorbed);
  for (size_t i = 0; i < all.size(); ++i)
    std::printf("region %zu %zu %016" PRIx64 " %016" PRIx64 "\n", i, all[i]->size(), hash_xyz(*all[i]), hash_rgb(*all[i]));
  std::printf("last %zu %016" PRIx64 "\n", last->size(), hash_xyz(*last));
  // segmentationregiongrow.cpp:87-106 with the façade's classes
  pcl::search::KdTree<PointTSeg>::Ptr tree(new pcl::search::KdTree<PointTSeg>);
  pcl::IndicesPtr indices(new std::vector<int>);
  pcl::PassThrough<PointTSeg> pass;
  pass.setInputCloud(frame);
  pass.setFilterFieldName("z");
  pass.setFilterLimits(0.0, 1.1);
  pass.filter(*indices);
  pcl::RegionGrowingRGB<PointTSeg> regRgb;
  regRgb.setInputCloud(frame);
  regRgb.setIndices(indices);
  regRgb.setSearchMethod(tree);
  regRgb.setDistanceThreshold(0.1);
  regRgb.setPointColorThreshold(10);
  regRgb.setRegionColorThreshold(10);
  regRgb.setMinClusterSize(700);
  std::vector<pcl::PointIndices> clusterIndices;
  regRgb.extract(clusterIndices);
  std::printf("classes %zu\n", clusterIndices.size());
  for (size_t i = 0; i < clusterIndices.size(); ++i) {
    Cloud cloudCluster;
    uint64_t hi = 1469598103934665603ull;
    for (int pit : clusterIndices[i].indices) { cloudCluster.points.push_back(frame->points[pit]); hi = fnv(hi, &pit, 4); }
    std::printf("class %zu %zu %016" PRIx64 " %016" PRIx64 "\n", i, cloudCluster.size(), hash_xyz(cloudCluster), hi);
  }
  return 0;
}
