// segmentation_check.cpp — ope::ObjectSegmentationPlane and the façade classes under it from a file, for
// tests/test_gpu_tabletop_pipeline.py:
//
//   segmentation_check <frame.pcd> [--except-plane]
//
// Prints, floats as their 32 bits in hex and point lists as an FNV-1a hash of their xyz bytes:
//   sac found <0|1> coeff <a> <b> <c> <d> inliers <n> hash <h>      getPlaneIndicesAndCoeffSAC (pcl::SACSegmentation)
//   extract plane <n> <h> rest <n> <h>                              getPlaneAndNonPlaneCloud (pcl::ExtractIndices)
//   minmax <min x> <min y> <max x> <max y>                          getProjectedCloud (pcl::ProjectInliers) + pcl::getMinMax3D
//   prism <n> hash <h>                                              pcl::ExtractPolygonalPrismData over the four corners (:174-214)
//   objects <0|1> plane <n> <h> clusters <k>                        getSegmentedObjectsOnPlane
//   cluster <i> <n> <h>                                             ... each cluster
// and with --except-plane, after them (the colours hashed as well: <hc> is the FNV-1a hash of the clusters' rgb words):
//   filtered <n> <h>                                                getFiltered
//   except planes <k> sizes <c0> ... rest <m> clusters <k>          getSegmentedObjectsExceptPlane
//   except cluster <i> <n> <h> <hc>                                 ... each cluster
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "object_segmentation_plane.hpp"
#include "pcd_io.hpp"

namespace pcl = ope::compat;
typedef ope::ObjectSegmentationPlane::PointTObj PointTObj;
typedef pcl::PointCloud<PointTObj> Cloud;

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

static uint64_t hash_xyz(const Cloud &c) {
  uint64_t h = 1469598103934665603ull;
  for (const PointTObj &p : c.points) {
    unsigned char b[12];
    std::memcpy(b, &p.x, 4); std::memcpy(b + 4, &p.y, 4); std::memcpy(b + 8, &p.z, 4);
    for (unsigned char v : b) { h ^= v; h *= 1099511628211ull; }
  }
  return h;
}

static uint64_t hash_rgb(const Cloud &c) {
  uint64_t h = 1469598103934665603ull;
  for (const PointTObj &p : c.points) {
    unsigned char b[4];
    std::memcpy(b, &p.rgb, 4);
    for (unsigned char v : b) { h ^= v; h *= 1099511628211ull; }
  }
  return h;
}

int main(int argc, char **argv) {
  const bool except = argc == 3 && std::strcmp(argv[2], "--except-plane") == 0;
  if (argc != 2 && !except) { std::fprintf(stderr, "usage: %s <frame.pcd> [--except-plane]\n", argv[0]); return 2; }
  Cloud::Ptr frame(new Cloud);
  if (pcl::io::loadPCDFile(argv[1], *frame) != 0) return 3;
  ope::ObjectSegmentationPlane seg;
  pcl::PointIndices::Ptr indices(new pcl::PointIndices);
  pcl::ModelCoefficients::Ptr coeff(new pcl::ModelCoefficients);
  const bool found = seg.getPlaneIndicesAndCoeffSAC(frame, indices, coeff);
  Cloud::Ptr plane(new Cloud), rest(new Cloud);
  seg.getPlaneAndNonPlaneCloud(frame, indices, plane, rest);
  std::printf("sac found %d coeff", found ? 1 : 0);
  for (float v : coeff->values) std::printf(" %08x", bits(v));
  std::printf(" inliers %zu hash %016" PRIx64 "\n", indices->indices.size(), hash_xyz(*plane));
  std::printf("extract plane %zu %016" PRIx64 " rest %zu %016" PRIx64 "\n", plane->size(), hash_xyz(*plane), rest->size(), hash_xyz(*rest));
  if (found) {
    Cloud::Ptr projected = seg.getProjectedCloud(frame, indices, coeff);
    PointTObj minPt, maxPt;
    pcl::getMinMax3D(*projected, minPt, maxPt);
    std::printf("minmax %08x %08x %08x %08x\n", bits(minPt.x), bits(minPt.y), bits(maxPt.x), bits(maxPt.y));
    // the four corners as objectsegmentationplane.cpp:174-188 writes them
    std::vector<float> vectorX, vectorY;
    vectorX.push_back(minPt.x - 0.1); vectorY.push_back(minPt.y - 0.1);
    vectorX.push_back(minPt.x - 0.1); vectorY.push_back(maxPt.y + 0.1);
    vectorX.push_back(maxPt.x + 0.1); vectorY.push_back(maxPt.y + 0.1);
    vectorX.push_back(maxPt.x + 0.1); vectorY.push_back(minPt.y - 0.1);
    const float a = coeff->values.at(0), b = coeff->values.at(1), c = coeff->values.at(2), d = coeff->values.at(3);
    Cloud::Ptr hull(new Cloud);
    hull->points.resize(4);
    for (int i = 0; i < 4; ++i) {
      const float x = vectorX.at(i), y = vectorY.at(i);
      volatile float ax = a * x, by = b * y;   // (each product rounded on its own)
      const float z = -((ax + by) + d) / c;
      hull->points[i].x = x; hull->points[i].y = y; hull->points[i].z = z;
    }
    hull->width = 4;
    pcl::PointIndices::Ptr cloudIndices(new pcl::PointIndices);
    pcl::ExtractPolygonalPrismData<PointTObj> extractPolyData;
    extractPolyData.setInputCloud(frame);
    extractPolyData.setInputPlanarHull(hull);
    extractPolyData.segment(*cloudIndices);
    Cloud inside;
    pcl::copyPointCloud(*frame, cloudIndices->indices, inside);
    std::printf("prism %zu hash %016" PRIx64 "\n", inside.size(), hash_xyz(inside));
  }
  std::vector<Cloud::Ptr> clusters;
  Cloud::Ptr cloudPlane;
  const bool ok = seg.getSegmentedObjectsOnPlane(frame, clusters, cloudPlane);
  std::printf("objects %d plane %zu %016" PRIx64 " clusters %zu\n", ok ? 1 : 0, cloudPlane->size(), hash_xyz(*cloudPlane), clusters.size());
  for (size_t i = 0; i < clusters.size(); ++i) std::printf("cluster %zu %zu %016" PRIx64 "\n", i, clusters[i]->size(), hash_xyz(*clusters[i]));
  if (except) {
    Cloud::Ptr filtered = seg.getFiltered(frame);
    std::printf("filtered %zu %016" PRIx64 "\n", filtered->size(), hash_xyz(*filtered));
    std::vector<Cloud::Ptr> objects = seg.getSegmentedObjectsExceptPlane(frame);
    if (seg.deviceFailed()) return 5;
    std::printf("except planes %d sizes", seg.lastPeel().n_planes);
    for (int32_t c : seg.lastPeelCounts()) std::printf(" %d", c);
    std::printf(" rest %d clusters %zu\n", seg.lastPeel().n_rest, objects.size());
    if (objects.size() != seg.deviceClusters().size()) return 6;
    for (size_t i = 0; i < objects.size(); ++i)
      std::printf("except cluster %zu %zu %016" PRIx64 " %016" PRIx64 "\n", i, objects[i]->size(), hash_xyz(*objects[i]), hash_rgb(*objects[i]));
  }
  return 0;
}
