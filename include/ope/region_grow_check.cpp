// region_grow_check.cpp — ope::SegmentationRegionGrow and compat::RegionGrowing from a file, for
// tests/test_gpu_region_grow_facade.py:
//
//   region_grow_check <frame.pcd>
//
// Prints, point lists as an FNV-1a hash of their xyz bytes and <hc> as that of their rgb words:
//   crop <n>                                     points the z crop over [0, 1.2] kept
//   regions <k> sweeps <s> one_way <e>           getSegmentRegGrow
//   region <i> <n> <h> <hc>                      ... each cluster (getClusters)
//   last <n> <h>                                 ... its return value
//   classes <k>                                  the same through PassThrough, NormalEstimation and RegionGrowing, as the reference
//   class <i> <n> <h>                            writes them (segmentationregiongrow.cpp:17-39), gathered from the cropped cloud
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
  Cloud::Ptr last = seg.getSegmentRegGrow(frame);
  if (seg.deviceFailed()) return 5;
  const auto &all = seg.getClusters();
  if (all.size() != seg.deviceClusters().size()) return 6;
  std::printf("crop %zu\n", seg.lastCropSize());
  std::printf("regions %zu sweeps %lld one_way %lld\n", all.size(), (long long)seg.lastStats().sweeps, (long long)seg.lastStats().one_way_edges);
  for (size_t i = 0; i < all.size(); ++i)
    std::printf("region %zu %zu %016" PRIx64 " %016" PRIx64 "\n", i, all[i]->size(), hash_xyz(*all[i]), hash_rgb(*all[i]));
  std::printf("last %zu %016" PRIx64 "\n", last->size(), hash_xyz(*last));
  // segmentationregiongrow.cpp:11-39 with the façade's classes
  pcl::search::KdTree<PointTSeg>::Ptr tree(new pcl::search::KdTree<PointTSeg>);
  pcl::PointCloud<pcl::Normal>::Ptr normals(new pcl::PointCloud<pcl::Normal>);
  Cloud::Ptr cloudFilteredZ(new Cloud);
  pcl::PassThrough<PointTSeg> pass;
  pass.setInputCloud(frame);
  pass.setFilterFieldName("z");
  pass.setFilterLimits(0.0, 1.2);
  pass.filter(*cloudFilteredZ);
  pcl::NormalEstimation<PointTSeg, pcl::Normal> normalEstimator;
  normalEstimator.setSearchMethod(tree);
  normalEstimator.setInputCloud(cloudFilteredZ);
  normalEstimator.setKSearch(30);
  normalEstimator.compute(*normals);
  pcl::RegionGrowing<PointTSeg, pcl::Normal> reg;
  reg.setMinClusterSize(500);
  reg.setMaxClusterSize(1000000);
  reg.setSearchMethod(tree);
  reg.setNumberOfNeighbours(15);
  reg.setInputCloud(cloudFilteredZ);
  reg.setInputNormals(normals);
  reg.setSmoothnessThreshold(10.0 / 180.0 * M_PI);
  reg.setCurvatureThreshold(1.0);
  std::vector<pcl::PointIndices> clusterIndices;
  reg.extract(clusterIndices);
  std::printf("classes %zu\n", clusterIndices.size());
  for (size_t i = 0; i < clusterIndices.size(); ++i) {
    Cloud cloudCluster;
    for (int pit : clusterIndices[i].indices) cloudCluster.points.push_back(cloudFilteredZ->points[pit]);
    std::printf("class %zu %zu %016" PRIx64 "\n", i, cloudCluster.size(), hash_xyz(cloudCluster));
  }
  return 0;
}
