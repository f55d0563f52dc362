// object_detection_check.cpp — ope::ObjectDetection and compat::VFHEstimation from files, for tests/test_gpu_vfh_facade.py:
//
//   object_detection_check <train_dir> <out_dir> <cluster.pcd>...
//
// <train_dir> holds training_data.list / training_data.f32.  Prints
//   models <m>                                   loadTrainData
//   name <i> <found> <name> <distance %.9g>      getObjectName of cluster i (the distance of neighbour [1])
//   batch <i> <name> <distance %.9g>             getObjectNames of all clusters in one call
//   vfh <i> <h>                                  FNV-1a hash of getVfhFeature's 308 floats
//   classes <i> <h>                              the same through NormalEstimation (k = 30) and VFHEstimation
//   rewritten <m>                                the table written again under <out_dir> by getkdTreeRepresentation and re-read
#include <cinttypes>
#include <cstdio>
#include <string>
#include <vector>

#include "object_detection.hpp"
#include "pcd_io.hpp"

namespace pcl = ope::compat;
typedef ope::ObjectDetection::PointTDet PointTDet;
typedef pcl::PointCloud<PointTDet> Cloud;

static uint64_t fnv(const void *p, size_t n) {
  uint64_t h = 1469598103934665603ull;
  const unsigned char *b = static_cast<const unsigned char *>(p);
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}

int main(int argc, char **argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: %s <train_dir> <out_dir> <cluster.pcd>...\n", argv[0]); return 2; }
  ope::ObjectDetection det;
  if (!det.loadTrainData(argv[1])) return 3;
  std::printf("models %zu\n", det.getModels().size());
  std::vector<Cloud::Ptr> clouds;
  std::vector<std::shared_ptr<pcl::CloudHandle>> dev;
  for (int a = 3; a < argc; ++a) {
    Cloud::Ptr c(new Cloud);
    if (pcl::io::loadPCDFile(argv[a], *c) != 0) return 4;
    clouds.push_back(c);
    dev.push_back(pcl::upload(*c, false));
    if (!dev.back()->h) return 5;
  }
  for (size_t i = 0; i < clouds.size(); ++i) {
    std::string name;
    const bool found = det.getObjectName(clouds[i], name);
    std::printf("name %zu %d %s %.9g\n", i, found ? 1 : 0, name.c_str(), det.lastDistance());
  }
  std::vector<std::string> names;
  std::vector<float> dist;
  if (!det.getObjectNames(dev, names, &dist)) return 6;
  for (size_t i = 0; i < names.size(); ++i) std::printf("batch %zu %s %.9g\n", i, names[i].c_str(), dist[i]);
  for (size_t i = 0; i < clouds.size(); ++i) {
    pcl::PointCloud<pcl::VFHSignature308>::Ptr vfh;
    det.getVfhFeature(clouds[i], vfh);
    if (!vfh || vfh->size() != 1) return 7;
    std::printf("vfh %zu %016" PRIx64 "\n", i, fnv(vfh->points[0].histogram, 308 * 4));
    // objectdetection.cpp:12-27 with the facade's classes
    pcl::PointCloud<pcl::Normal>::Ptr normals(new pcl::PointCloud<pcl::Normal>);
    pcl::search::KdTree<PointTDet>::Ptr kdTree(new pcl::search::KdTree<PointTDet>);
    pcl::NormalEstimation<PointTDet, pcl::Normal> normEst;
    normEst.setInputCloud(clouds[i]);
    normEst.setSearchMethod(kdTree);
    normEst.setKSearch(30);
    normEst.compute(*normals);
    pcl::VFHEstimation<PointTDet, pcl::Normal, pcl::VFHSignature308> vfhEst;
    pcl::PointCloud<pcl::VFHSignature308> out;
    vfhEst.setInputCloud(clouds[i]);
    vfhEst.setInputNormals(normals);
    vfhEst.setSearchMethod(kdTree);
    vfhEst.compute(out);
    if (out.size() != 1) return 8;
    std::printf("classes %zu %016" PRIx64 "\n", i, fnv(out.points[0].histogram, 308 * 4));
  }
  // the training stage: the same models written again and read back
  ope::ObjectDetection again;
  for (const ope::vfhModel &m : det.getModels()) again.addModel(m.first, m.second.data());
  if (!again.getkdTreeRepresentation(argv[2])) return 9;
  ope::ObjectDetection third;
  if (!third.loadTrainData(argv[2])) return 10;
  std::printf("rewritten %zu\n", third.getModels().size());
  return 0;
}
